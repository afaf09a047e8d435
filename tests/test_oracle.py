"""CPU tests: the oracle restatement against (a) the committed golden vectors made by the
reference's own models.py, (b) what the reference computes on small cases, recorded by running it in place
(oracle/make_reference_records.py -> tests/golden/reference_records.*), and (c) the substitute pins of
SURVEY.md section 8c (param counts, key sets, zero-init identity)."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file

from oracle import cases, unet_ref
from oracle import controllora_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = list(cases.CASES) + ["lora"]


@pytest.mark.parametrize("case", ALL_CASES)
def test_oracle_matches_golden(case, golden_dir):
    gold = load_file(os.path.join(golden_dir, f"case_{case}.safetensors"))
    unet, params, fwd = cases.build_oracle_case(case)
    assert torch.allclose(cases.weight_checksum(unet), gold["unet_checksum"], rtol=1e-12), "seeded UNet weights drifted"
    assert torch.allclose(cases.weight_checksum(params), gold["clora_checksum"], rtol=1e-12), "seeded adapter weights drifted"
    out = cases.oracle_train_step(unet, params, fwd, cases.seeded_inputs())
    for k, v in out.items():
        ref = gold[k]
        err = float((v - ref).norm() / (ref.norm() + 1e-30))
        assert err < 2e-5, f"{case}:{k} rel-L2 {err:.3e}"


def chain_modules(impl, case, cad):
    """(control processor, pre LoRA, post LoRA) of `impl` (the reference's models module or oracle.controllora_ref)"""
    if impl is cr:
        proc = (cr.ControlLoRAProcRef(64, cad, rank=4) if case == "v1" else
                cr.ControlLoRAProcV2Ref(64, cad, rank=4, control_channels=32))
        return proc, cr.LoRAProcRef(64, cad, rank=4), cr.LoRAProcRef(64, cad, rank=2, post_add=True)
    proc = (impl.ControlLoRACrossAttnProcessor(64, cad, rank=4) if case == "v1" else
            impl.ControlLoRACrossAttnProcessorV2(64, cad, rank=4, control_channels=32))
    return proc, impl.LoRACrossAttnProcessor(64, cad, rank=4), impl.LoRACrossAttnProcessor(64, cad, rank=2, post_add=True)


@pytest.mark.parametrize("case", ["v1", "v2"])
def test_oracle_matches_reference_with_adapter_chain(case, golden_dir):
    """pre_loras / post_loras chaining (reference models.py:232-243, 249-265, 276-282;
    mix_lora_and_control_lora.py:111-123) -- restatement vs the reference's output recorded in place
    with the same weights and inputs (oracle/make_reference_records.py)."""
    rec = load_file(os.path.join(golden_dir, "reference_records.safetensors"))
    for self_attn in (True, False):
        head = f"chain.{case}.{'self' if self_attn else 'cross'}."
        part = lambda name: {k[len(head + name) + 1:]: v for k, v in rec.items() if k.startswith(head + name + ".")}
        cad = None if self_attn else 48
        attn = unet_ref.CrossAttention(64, cad, heads=4, dim_head=16)
        attn.load_state_dict(part("attn"))
        b, pre_b, post_b = chain_modules(cr, case, cad)
        b.load_state_dict(part("proc")); pre_b.load_state_dict(part("pre")); post_b.load_state_dict(part("post"))
        b.inject_pre_lora(pre_b); b.inject_post_lora(post_b)
        b.inject_control_states(rec[head + "ctrl"].clone())
        yb = b(attn, rec[head + "h"], None if self_attn else rec[head + "e"], None, 0.7)
        ya = rec[head + "y"]
        assert ya.shape == yb.shape and torch.allclose(ya, yb, atol=1e-6), float((ya - yb).abs().max())


@pytest.mark.parametrize("name,n_params,n_keys", [
    ("fill50k", 6047040, 400), ("diffusiondb-canny", 6047040, 400), ("mpii-pose", 6047040, 400),
    ("post-add", 6048576, 400), ("danbooru-sketch", 19810304, 376),
    ("mpii-pose-v2", 5000704, 312), ("diffusiondb-canny-v2", 5000704, 312)])
def test_param_counts_and_keys_vs_reference_configs(name, n_params, n_keys, golden_dir):
    """the reference's ControlLoRA built from its own configs/<name>.json (recorded in place: parameter count, state-dict keys
    and shapes) vs the restatement built from this repository's copy of that config"""
    with open(os.path.join(golden_dir, "reference_records.json")) as f:
        ref = json.load(f)[f"configs.{name}"]
    path = os.path.join(ROOT, "configs", f"{name}.json")
    with open(path) as f:
        assert json.load(f) == ref["config"]
    b = cr.ControlLoRARef.from_config(path)
    assert sum(p.numel() for p in b.parameters()) == n_params == ref["n_params"]
    shapes = {k: list(v.shape) for k, v in b.state_dict().items()}
    assert shapes == ref["state_dict_shapes"] and len(shapes) == n_keys


def test_sd15_unet_parameter_count():
    with torch.device("meta"):
        u = unet_ref.UNet2DConditionModel()
    assert sum(p.numel() for p in u.parameters()) == 859_520_964
    assert len(u.attn_processors) == 32


@pytest.mark.parametrize("case", ["v1", "v2"])
def test_zero_init_identity(case):
    """a freshly initialised ControlLoRA leaves the UNet output bit-identical."""
    torch.manual_seed(0)
    unet = unet_ref.UNet2DConditionModel(**cases.SMALL_UNET)
    cases.seeded_weights_(unet, seed=11)
    inp = cases.seeded_inputs()
    with torch.no_grad():
        plain = unet(inp["latents"], inp["timesteps"], inp["ehs"]).sample
        clora = cr.ControlLoRARef(**cases.CASES[case])       # default init: every `up` is zero
        unet.set_attn_processor(cr.map_processors_to_unet(unet, clora))
        clora(inp["guide"])
        with_adapters = unet(inp["latents"], inp["timesteps"], inp["ehs"]).sample
    assert torch.equal(plain, with_adapters)


def test_mapping_order():
    """M1: lora_layers[i][0..3] -> down_blocks.i, [4..9] -> up_blocks.(3-i), lora_layers[3] -> mid."""
    unet = unet_ref.UNet2DConditionModel(**cases.SMALL_UNET)
    clora = cr.ControlLoRARef(**cases.SMALL_CLORA_V1)
    m = cr.map_processors_to_unet(unet, clora)
    assert m["down_blocks.1.attentions.0.transformer_blocks.0.attn2.processor"] is clora.lora_layers[1][1]
    assert m["up_blocks.3.attentions.2.transformer_blocks.0.attn1.processor"] is clora.lora_layers[0][8]
    assert m["mid_block.attentions.0.transformer_blocks.0.attn2.processor"] is clora.lora_layers[3][1]
    assert m["up_blocks.1.attentions.0.transformer_blocks.0.attn1.processor"] is clora.lora_layers[2][4]


def test_ddim_timesteps():
    s = unet_ref.DDPMSchedule()
    ts = s.ddim_timesteps(50)
    assert ts[0] == 981 and ts[-1] == 1 and len(ts) == 50


def test_dpm_solver_pp_identities():
    """DPM-Solver++(2M) (the sampler of the reference apps) restated without upstream diffusers: pin what must hold.
    (1) its first-order update is the DDIM(eta=0) update between the same two timesteps;
    (2) a model whose epsilon is consistent with ONE fixed x0 is integrated exactly by the first AND second order updates."""
    import torch
    from controllora_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler
    torch.manual_seed(0)
    x = torch.randn(2, 4, 8, 8, dtype=torch.float64)
    eps = torch.randn_like(x)
    dpm = DPMSolverMultistepScheduler(solver_order=1)
    dpm.set_timesteps(20)
    t, prev = dpm.timesteps[3], dpm.timesteps[4]
    ddim = DDIMScheduler()
    a_t, a_p = float(ddim.alphas_cumprod[t]), float(ddim.alphas_cumprod[prev])
    x0 = (x - (1 - a_t) ** 0.5 * eps) / a_t ** 0.5
    ref = a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * eps
    assert float((dpm.step(eps, t, x) - ref).abs().max()) < 1e-6
    for order in (1, 2):
        s = DPMSolverMultistepScheduler(solver_order=order)
        s.set_timesteps(12)
        target = torch.randn(1, 4, 8, 8, dtype=torch.float64)
        t0 = s.timesteps[0]
        lat = float(s._alpha[t0]) * target + float(s._sigma[t0]) * torch.randn_like(target)
        for t in s.timesteps:
            e = (lat - float(s._alpha[t]) * target) / float(s._sigma[t])       # the exact-x0 "model"
            lat = s.step(e, t, lat)
            nxt = s.timesteps[s.timesteps.index(t) + 1] if t != s.timesteps[-1] else 0
            # every update keeps the trajectory on {alpha x0 + sigma eps}: the same eps explains the new latent
            assert float((lat - float(s._alpha[nxt]) * target - float(s._sigma[nxt]) * e).abs().max()) < 1e-5   # the update runs in fp32


def test_velocity_target_and_add_noise_are_consistent():
    """v-prediction target (reference train...:776-777): with x_t = a x0 + s eps and v = a eps - s x0 (a^2 + s^2 = 1),
    x0 = a x_t - s v and eps = s x_t + a v"""
    import torch
    from controllora_amd.schedulers import DDPMScheduler
    torch.manual_seed(1)
    sch = DDPMScheduler()
    x0, eps = torch.randn(3, 4, 8, 8, dtype=torch.float64), torch.randn(3, 4, 8, 8, dtype=torch.float64)
    t = torch.tensor([0, 500, 999])
    xt, v = sch.add_noise(x0, eps, t), sch.get_velocity(x0, eps, t)
    a = sch.alphas_cumprod.double()[t].sqrt().reshape(-1, 1, 1, 1)
    s = (1 - sch.alphas_cumprod.double()[t]).sqrt().reshape(-1, 1, 1, 1)
    assert float((a * xt - s * v - x0).abs().max()) < 1e-6 and float((s * xt + a * v - eps).abs().max()) < 1e-6


def test_fp16_noise_floor_of_the_ddim_loop():
    """Tolerance reading of north_star's "denoised latents ... within 1e-3 rel fp16" (SURVEY.md section 8c): the oracle's
    OWN 50-step DDIM + CFG loop run in fp16 storage (the arithmetic regime of the reference's fp16 pipeline) sits several
    1e-3 (rel-L2) away from the same loop in fp32 -- no fp16 implementation, the reference's included, is within 1e-3 of
    the fp32 path.  The GPU suite asserts the product's error against this floor (tests/test_full_topology_gpu.py)."""
    from tests import full_cases as F
    o_unet, _, o_clora = cases.build_oracle_case("v1")
    with torch.no_grad():
        for p in o_unet.parameters():
            p.copy_(p.half().float())
    g = torch.Generator().manual_seed(5)
    guide = ((torch.rand(1, 3, 128, 128, generator=g) > 0.9).float() * 2 - 1)
    cond = torch.randn(2, 7, 64, generator=g).half().float()
    uncond = torch.randn(2, 7, 64, generator=g).half().float()
    lat0 = torch.randn(2, 4, 16, 16, generator=g).half().float()
    ref, _ = F.oracle_ddim(o_unet, o_clora, guide, cond, uncond, 50, 9.0, lat0)
    floor = F.fp16_oracle_floor(o_unet, o_clora, guide, cond, uncond, 50, 9.0, lat0, ref)
    print("fp16 oracle vs fp32 oracle, 50-step DDIM latents rel-L2:", floor)
    assert 1e-3 < floor < 2e-2
