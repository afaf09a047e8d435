"""-m gpu: the one-launch sampler step on the real library -- the kernel cases of tests/sampler_step_cases.py, and
pipeline.ddim_sample(step_impl="device") on the small product topology of tests/e2e_cases at 64 x 64 pixels: teacher-forced against
the fp64 host schedulers, the replayed graph against the eager loop, eta = 0 against no eta.  No CPU oracle UNet runs here."""
import functools

import pytest
import torch

from tests import sampler_step_cases as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", S.COEF_SETS)
@pytest.mark.parametrize("layout", S.LAYOUTS)
@pytest.mark.parametrize("shape", [s for s in S.SHAPES if s != S.PAST_CAP])
def test_step_against_fp64(shape, layout, name):
    S.check_step(shape, layout, name, "cuda")


@pytest.mark.parametrize("name", S.PAST_CAP_SETS)
@pytest.mark.parametrize("layout", S.LAYOUTS)
def test_step_past_the_grid_cap_against_fp64(layout, name):
    S.check_step(S.PAST_CAP, layout, name, "cuda")


@pytest.mark.parametrize("layout", S.LAYOUTS)
@pytest.mark.parametrize("shape", [(3, 4, 5, 7), (2, 4, 64, 64)])
def test_step_properties(shape, layout):
    S.check_properties(shape, layout, "cuda")


def test_step_argument_errors():
    S.check_argument_errors("cuda")


def test_step_reads_the_view_the_unet_returns():
    """the UNet's own output -- the permuted view of the padded conv_out rows -- goes to the kernel as it is: same bits as its dense copy"""
    model, inp = _model()
    x_in = torch.cat([inp["latents"], inp["latents"]], 0).half()
    with torch.no_grad():
        model["control"](inp["guide"])
        eps = model["unet"](x_in, 500, torch.cat([inp["uncond"], inp["cond"]], 0)).sample
    assert not eps.is_contiguous() and eps.stride(1) == 1, eps.stride()
    x, hist, noise = S.make_state(tuple(inp["latents"].shape), "cuda")
    a = S.launch(eps, x, hist, noise, S.coef_sets()["dpm_second"])
    b = S.launch(eps.contiguous(), x, hist, noise, S.coef_sets()["dpm_second"])
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@functools.lru_cache(maxsize=None)
def _model():
    """the small product topology with a v1 ControlLoRA, and the inputs of a 2-image run at 64 x 64 pixels (8 x 8 latents, UNet batch 4,
    one guide broadcast over the batch): built once, never modified"""
    from tests.e2e_cases import build_product_case
    torch.manual_seed(0)
    unet, _, clora = build_product_case("v1", "cuda")
    g = torch.Generator().manual_seed(21)
    inp = dict(guide=(torch.rand(1, 3, 64, 64, generator=g) * 2 - 1).half().cuda(), cond=torch.randn(2, 77, 64, generator=g).half().cuda(),
               uncond=torch.randn(2, 77, 64, generator=g).half().cuda(), latents=torch.randn(2, 4, 8, 8, generator=g).half().cuda())
    return dict(unet=unet, control=clora), inp


def _run(name, **kw):
    model, inp = _model()
    return S.run_loop(name, model["unet"], model["control"], **inp, **kw)[0]


@pytest.mark.parametrize("name", sorted(S.LOOPS))
def test_device_loop_teacher_forced(name):
    model, inp = _model()
    S.check_teacher_forced(name, model["unet"], model["control"], **inp)


@pytest.mark.parametrize("name", sorted(S.LOOPS))
def test_replayed_graph_is_the_eager_loop_bit_for_bit(name):
    eager, graphed = _run(name, graph=False), _run(name, graph=True)
    assert torch.isfinite(eager).all()
    assert torch.equal(eager, graphed), f"{int((eager != graphed).sum())} of {eager.numel()} final latents differ"


def test_eta_zero_is_the_loop_without_eta():
    for graph in (False, True):
        assert torch.equal(_run("ddim8", graph=graph), _run("ddim8", graph=graph, eta=0.0))
    assert torch.equal(_run("dpm8", graph=True), _run("dpm8", graph=True, eta=0.7))          # DPM-Solver++ ignores eta


@pytest.mark.parametrize("name", sorted(S.LOOPS))
def test_device_loop_against_host_loop_is_reported(name):
    """fp32 summation order, amplified through the fp16 UNet input: printed (tools/sampler_step_bench.py reports the same figure at
    512 x 512), not asserted beyond finiteness"""
    dev, host = _run(name, graph=True), _run(name, graph=True, step_impl="host")
    err = float((dev - host).norm() / host.norm())
    print(f"SAMPLER_LOOP {name}: device against host final latents rel-L2 {err:.3e}")
    assert torch.isfinite(dev).all() and torch.isfinite(host).all()


def test_pipeline_passes_eta_and_step_impl_through():
    from controllora_amd import models as M
    from controllora_amd.pipeline import ControlLoRAPipeline
    from oracle import cases
    torch.manual_seed(0)
    pipe = ControlLoRAPipeline.from_pretrained("random:small", M.ControlLoRA(**cases.SMALL_CLORA_V1), "cuda")
    guide = torch.rand(1, 3, 64, 64) * 2 - 1
    kw = dict(num_samples=2, ddim_steps=8, scale=7.5, seed=5)
    a = pipe("red circle", guide, step_impl="device", **kw)
    b = pipe("red circle", guide, step_impl="device", eta=0.0, **kw)
    c = pipe("red circle", guide, step_impl="device", eta=1.0, **kw)
    d = pipe("red circle", guide, step_impl="host", eta=1.0, **kw)
    assert a.shape == (2, 64, 64, 3) and torch.equal(a, b) and not torch.equal(a, c)
    print("SAMPLER_PIPELINE eta = 1: mean |device - host| (uint8 levels):", float((c.int() - d.int()).abs().float().mean()))
    with pytest.raises(ValueError, match="step_impl"):
        pipe("red circle", guide, step_impl="fused", **kw)
