"""-m gpu: the DreamBooth-LoRA path on the real library -- the per-sample-weighted MSE launch, the plain-LoRA trainer step
(prior preservation against the oracle, the plain step against the reference's golden, graph replay against eager steps), and
the entry point end to end: class images, checkpoints, resume, and the LoRA file mixed into a ControlLoRA and sampled."""
import json
import os

import pytest
import torch

from tests import dreambooth_cases as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,n", D.KERNEL_SHAPES)
def test_weighted_mse_with_unit_weights_is_the_plain_mse(B, n):
    D.check_unit_weights_equal_plain_mse(B, n, "cuda")


@pytest.mark.parametrize("B,n", D.KERNEL_SHAPES)
def test_weighted_mse_mixed_weights_against_fp64(B, n):
    D.check_mixed_weights_against_fp64(B, n, "cuda")


def test_weighted_mse_argument_errors():
    D.check_argument_errors("cuda")


def test_prior_preservation_step_matches_oracle_autograd():
    D.check_prior_preservation_step("cuda")


def test_plain_step_through_the_lora_trainer_matches_reference_golden(golden_dir):
    D.check_plain_step_against_golden("cuda", golden_dir)


def test_graph_replay_matches_eager_prior_preservation_steps():
    """tests/test_e2e_gpu.py::test_graph_replay_matches_eager_step's comparison and limits, on the weighted step, 3 steps"""
    from controllora_amd import ops
    out = []
    for graphed in (False, True):
        torch.manual_seed(0)
        tr = D.make_trainer("cuda")
        args, w = D.step_args("cuda", 4), D.prior_weights("cuda")
        start = tr.flat.data.clone()
        if graphed:
            tr.capture(*args, w, warmup=1)           # warm-up steps move the parameters: restore them
            tr.flat.data.copy_(start); tr.flat.exp_avg.zero_(); tr.flat.exp_avg_sq.zero_(); tr.state[2] = 0
            ops.repack_adapters()
            for _ in range(3):
                tr.step_graphed(*args)
        else:
            for _ in range(3):
                tr.step(*args, w)
        torch.cuda.synchronize()
        out.append((tr.flat.data.clone(), tr.loss(), tr.loss_parts(), float(tr.state[2])))
    (p0, l0, parts0, s0), (p1, l1, parts1, s1) = out
    assert s0 == s1 == 3.0
    assert abs(l0 - l1) < 1e-5 * max(1.0, abs(l0))
    assert all(abs(a - b) < 1e-5 * max(1.0, abs(a)) for a, b in zip(parts0, parts1))
    assert float((p0 - p1).norm() / p0.norm()) < 1e-5
    assert float((p0 - start).abs().max()) > 0


def test_pipeline_samples_without_a_control_model():
    from controllora_amd.pipeline import ControlLoRAPipeline
    pipe = ControlLoRAPipeline.from_pretrained("random:small", None)
    img = pipe("a photo of a dog", num_samples=2, ddim_steps=2, scale=7.5, seed=1, height=64, width=128)
    assert img.shape == (2, 64, 128, 3) and img.dtype == torch.uint8
    again = pipe("a photo of a dog", None, num_samples=2, ddim_steps=2, scale=7.5, seed=1, height=64, width=128)
    assert torch.equal(img, again)
    with pytest.raises(ValueError):
        pipe("a photo of a dog", height=65)


def test_short_run_class_images_checkpoints_resume_and_mixing(tmp_path):
    import numpy as np
    from PIL import Image
    from controllora_amd import loading, models as M
    from controllora_amd.pipeline import ddim_sample
    from tests.e2e_cases import build_product_case
    import train_dreambooth_lora as T
    inst = tmp_path / "instance"
    os.makedirs(inst)
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 255, (80, 72, 3), dtype=np.uint8)).save(inst / f"{i}.png")
    out, cls = tmp_path / "run", tmp_path / "class"
    common = ["--pretrained_model_name_or_path", "random:small", "--instance_data_dir", str(inst), "--instance_prompt", "a photo of sks dog",
              "--class_data_dir", str(cls), "--class_prompt", "a photo of a dog", "--with_prior_preservation", "--prior_loss_weight", "0.5",
              "--num_class_images", "2", "--resolution", "64", "--train_batch_size", "2", "--checkpointing_steps", "2",
              "--validation_prompt", "a photo of sks dog", "--num_validation_images", "1", "--seed", "3", "--output_dir", str(out)]
    assert T.main(common + ["--max_train_steps", "4"]) == 4
    names = sorted(os.listdir(cls))
    assert len(names) == 2 and all(n.endswith(".jpg") and len(n.split("-")[1]) == 40 + 4 for n in names), names
    assert sorted(n.split("-")[0] for n in names) == ["0", "1"]
    assert os.path.isdir(out / "checkpoint-2") and os.path.isdir(out / "checkpoint-4")
    assert os.path.exists(out / "pytorch_lora_weights.bin") and os.path.exists(out / "pytorch_lora_weights.safetensors")
    assert len(os.listdir(out / "validation")) >= 1
    log = [json.loads(l) for l in open(out / "logs" / "train_log.jsonl")]
    assert log and all(np.isfinite(r[k]) for r in log for k in ("step_loss", "instance_loss", "prior_loss"))
    assert all(abs(r["step_loss"] - (r["instance_loss"] + 0.5 * r["prior_loss"])) < 1e-5 * r["step_loss"] for r in log)
    assert T.main(common + ["--max_train_steps", "6", "--resume_from_checkpoint", "latest", "--no_hipgraph"]) == 6
    assert os.path.isdir(out / "checkpoint-6") and len(os.listdir(cls)) == 2
    sd = loading._read_lora_file(str(out))
    ups = [v for k, v in sd.items() if k.endswith("to_q_lora.up.weight")]
    assert ups and any(float(v.abs().max()) > 0 for v in ups)                      # zero-init `up` has moved
    # the loop closed: the file loads, mixes into a small ControlLoRA, folds, and samples
    unet, _, clora = build_product_case("v1", "cuda")
    M.mix_lora_into_control_lora(unet, clora, loading.load_lora_attn_procs(unet, str(out)), pre=True, post=False, fold=True)
    clora.fold_chains(True)
    rep = clora.fold_report()
    assert rep and all(r["folded"] for r in rep.values()), rep
    from oracle import cases
    inp = {k: v.cuda() for k, v in cases.seeded_inputs().items()}
    lat = ddim_sample(unet, clora, inp["guide"][:1].half(), inp["ehs"][:1].half(), inp["ehs"][1:2].half(), steps=2, guidance_scale=7.5,
                      latents=inp["latents"][:1].half(), sampler="dpm")
    assert lat.shape == (1, 4, 16, 16) and torch.isfinite(lat).all()


def test_short_last_batch_between_graph_replays_logs_what_an_eager_run_logs(tmp_path):
    """3 instance and 3 class images at batch 2 over 2 epochs: the UNet batches are 4, 2, 4, 2 -- the short one runs as an eager step
    between replays of the captured step.  Every logged loss figure of the graphed run equals the eager run's
    (tests/test_e2e_gpu.py::test_graph_replay_matches_eager_step's limit), so no replay reports or writes another step's sums."""
    import numpy as np
    from PIL import Image
    import train_dreambooth_lora as T
    rng = np.random.default_rng(1)
    for name in ("instance", "class"):
        os.makedirs(tmp_path / name)
        for i in range(3):
            Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8)).save(tmp_path / name / f"{i}.png")
    logs = {}
    for tag, extra in (("graph", []), ("eager", ["--no_hipgraph"])):
        out = tmp_path / tag
        args = ["--pretrained_model_name_or_path", "random:small", "--instance_data_dir", str(tmp_path / "instance"), "--instance_prompt",
                "a photo of sks dog", "--class_data_dir", str(tmp_path / "class"), "--class_prompt", "a photo of a dog",
                "--with_prior_preservation", "--prior_loss_weight", "0.5", "--num_class_images", "3", "--resolution", "64", "--center_crop",
                "--train_batch_size", "2", "--num_train_epochs", "2", "--seed", "5", "--output_dir", str(out)] + extra
        assert T.main(args) == 4
        logs[tag] = [json.loads(l) for l in open(out / "logs" / "train_log.jsonl")]
    assert len(os.listdir(tmp_path / "class")) == 3
    assert [r["batch"] for r in logs["graph"]] == [r["batch"] for r in logs["eager"]] == [4, 2, 4, 2]
    for g, e in zip(logs["graph"], logs["eager"]):
        for k in ("step_loss", "instance_loss", "prior_loss"):
            print(f"SHORT_BATCH step {g['step']} batch {g['batch']} {k}: graph {g[k]!r} eager {e[k]!r}")
    for g, e in zip(logs["graph"], logs["eager"]):
        for k in ("step_loss", "instance_loss", "prior_loss"):
            assert abs(g[k] - e[k]) < 1e-5 * max(1.0, abs(e[k])), (g["step"], k, g[k], e[k])
        assert abs(g["step_loss"] - (g["instance_loss"] + 0.5 * g["prior_loss"])) < 1e-5 * g["step_loss"]
    losses = [r["step_loss"] for r in logs["graph"]]
    assert len(set(losses)) == 4, "every step saw other noise: four different losses"


# ---- a ladder under the short-last-batch test: which component stops repeating itself.  Rungs 1 and 2 are the two components of a
# step on their own (the VAE encoder, whose 64x64 and 32x32 norms are the only team GroupNorm launches at resolution 64, and one eager
# trainer step); rungs 3 and 4 separate "the run does not repeat itself" from "the graphed run differs from the eager one".
class _Outputs:
    """forward hooks that keep a copy of every submodule's output tensor in call order; first_difference() names the first module
    whose output differs between two recordings (= the launch to look at)"""

    def __init__(self, root):
        self.root, self.records, self.handles = root, [], []

    def __enter__(self):
        for name, mod in self.root.named_modules():
            if name:
                self.handles.append(mod.register_forward_hook(lambda m, i, o, name=name: self._keep(name, o)))
        return self

    def _keep(self, name, out):
        from controllora_amd import kernels as K
        # the output of a deferred split-K GEMM is unwritten until its consumer folds the slabs (kernels._PENDING): nothing to read yet
        if torch.is_tensor(out) and out.data_ptr() not in K._PENDING:
            self.records.append((name, out.detach().clone()))

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()
        return False

    def first_difference(self, other):
        assert [n for n, _ in self.records] == [n for n, _ in other.records]
        for (name, a), (_, b) in zip(self.records, other.records):
            if not torch.equal(a, b):
                return f"{name} {tuple(a.shape)}: {int((a != b).sum())} of {a.numel()} elements differ, rel {D.rel(a, b):.2e}"
        return None


@pytest.mark.parametrize("gn_team", [None, 0])
def test_ladder_1_vae_encode_repeats_itself_around_a_short_batch(gn_team):
    """moments of 4 images, of 2 of them, of the 4 again (team norms of 64, 128, 64 members over the same exchange state): the first
    and the third are the same bits, and every encoder module's output is; the same with the team kernels off"""
    from controllora_amd import kernels as K, loading
    from tests import kernel_cases as KC
    vae = loading.load_vae("random:small", "cuda")
    x = (torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(5)) * 2 - 1).half().cuda()
    before = KC.team_generations("cuda")
    with KC.options(gn_team=KC.option_default("gn_team") if gn_team is None else gn_team):
        runs = []
        for batch in (x, x[:2].contiguous(), x):
            with _Outputs(vae.encoder) as rec:
                dist = vae.encode(batch).latent_dist
            runs.append((rec, dist.mean.clone(), dist.logvar.clone()))
    moved = [a - b for a, b in zip(KC.team_generations("cuda"), before)]
    if gn_team == 0:
        assert moved == [0] * 32, moved
    else:       # per encode: two 64x64x16 norms, the 32x32x16 and the 32x32x32 one = 4 team launches of B units
        assert moved == [12] * 2 + [8] * 2 + [0] * 28, f"the encoder's norms did not take the team plan the test is about: {moved}"
    diff = runs[0][0].first_difference(runs[2][0])
    assert diff is None, f"first encoder output that differs between the two batch-4 passes: {diff}"
    assert torch.equal(runs[0][1], runs[2][1]) and torch.equal(runs[0][2], runs[2][2])
    print(f"LADDER_1 gn_team={gn_team}: moments of the batch of 2 against the first 2 of the batch of 4: rel {D.rel(runs[1][1], runs[0][1][:2]):.2e}")
    assert K.gn_team_errors("cuda") == 0


def test_ladder_2_one_eager_step_repeats_itself_in_a_fresh_trainer():
    """one eager batch-4 prior-preservation step from the same seed in two fresh trainers: loss parts and the flat gradient are the
    same bits, and every UNet module's output is"""
    out = []
    for _ in range(2):
        torch.manual_seed(0)
        tr = D.make_trainer("cuda")
        with _Outputs(tr.unet) as rec:
            tr.forward_backward(*D.step_args("cuda", 4), D.prior_weights("cuda"))
        torch.cuda.synchronize()
        out.append((rec, tr.loss_parts(), tr.loss(), tr.flat.grad.detach().clone()))
    diff = out[0][0].first_difference(out[1][0])
    assert diff is None, f"first UNet output that differs between two identical eager steps: {diff}"
    assert out[0][1] == out[1][1] and out[0][2] == out[1][2], (out[0][1:3], out[1][1:3])
    assert torch.equal(out[0][3], out[1][3]), f"flat.grad differs in {int((out[0][3] != out[1][3]).sum())} elements"


def _short_batch_logs(tmp_path, extra):
    """the 4, 2, 4, 2 run of the short-last-batch test, twice with the same arguments: the logged loss figures of both"""
    import numpy as np
    from PIL import Image
    import train_dreambooth_lora as T
    rng = np.random.default_rng(1)
    for name in ("instance", "class"):
        os.makedirs(tmp_path / name)
        for i in range(3):
            Image.fromarray(rng.integers(0, 255, (64, 64, 3), dtype=np.uint8)).save(tmp_path / name / f"{i}.png")
    logs = []
    for tag in ("first", "second"):
        out = tmp_path / tag
        args = ["--pretrained_model_name_or_path", "random:small", "--instance_data_dir", str(tmp_path / "instance"), "--instance_prompt",
                "a photo of sks dog", "--class_data_dir", str(tmp_path / "class"), "--class_prompt", "a photo of a dog",
                "--with_prior_preservation", "--prior_loss_weight", "0.5", "--num_class_images", "3", "--resolution", "64", "--center_crop",
                "--train_batch_size", "2", "--num_train_epochs", "2", "--seed", "5", "--output_dir", str(out)] + extra
        assert T.main(args) == 4
        logs.append([json.loads(l) for l in open(out / "logs" / "train_log.jsonl")])
    assert [r["batch"] for r in logs[0]] == [r["batch"] for r in logs[1]] == [4, 2, 4, 2]
    for a, b in zip(*logs):
        for k in ("step_loss", "instance_loss", "prior_loss"):
            print(f"LADDER {' '.join(extra) or 'graphed'} step {a['step']} batch {a['batch']} {k}: first {a[k]!r} second {b[k]!r}")
    for a, b in zip(*logs):
        for k in ("step_loss", "instance_loss", "prior_loss"):
            assert a[k] == b[k], (extra, a["step"], k, a[k], b[k])


def test_ladder_3_the_eager_short_batch_run_repeats_itself(tmp_path):
    _short_batch_logs(tmp_path, ["--no_hipgraph"])


def test_ladder_4_the_graphed_short_batch_run_repeats_itself(tmp_path):
    _short_batch_logs(tmp_path, [])
