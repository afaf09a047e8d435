"""CPU tests of mixing several ControlLoRAs, on the emulated kernels: the recorded reference outputs of chains with control
members, the control-mix kernel (clora_control_mix_q_f16) against fp64, the fused v1 site against the oracle chain, switches and
fallbacks, stale-job behaviour, broadcast of a batch-1 control map, and a whole small UNet steered by two control models."""
import copy

import pytest
import torch

from controllora_amd import capi, kernels as K, models as M
from oracle import cases
from tests import multi_control_cases as MC
from tests.emu_fixture import use_emulator

f16, f32 = torch.float16, torch.float32


@pytest.fixture(autouse=True)
def _emu():
    with use_emulator():
        yield


# ------------------------------------------------------------------------------------------------ 1. records
@pytest.fixture(scope="module")
def records():
    return MC.load_records()


def test_records_cover_every_case(records):
    assert sorted(records) == sorted(f"{c}:{w}:cb{b}" for c in MC.RECORD_CASES for w in ("self", "cross") for b in (1, 2))
    for name, rec in records.items():
        assert {"h", "y", "ctrl.main", "main.to_q_lora.up.weight", "attn.to_q.weight"} <= set(rec), name
        assert ("e" in rec) == (":cross:" in name) and any(k.startswith("ctrl.member") for k in rec), name


def test_oracle_restatement_reproduces_the_records(records):
    """the limit tests/test_oracle.py applies to the chain.* records"""
    for name, rec in records.items():
        yb, ya = MC.replay_record(name, rec, "oracle")
        assert ya.shape == yb.shape and torch.allclose(ya, yb, atol=1e-6), (name, float((ya - yb).abs().max()))


def test_generic_path_reproduces_the_records(records):
    for name, rec in records.items():
        y, ya = MC.replay_record(name, rec, "product")
        e = MC.rel(y, ya)
        print(f"MULTI_CONTROL_RECORD {name}: generic path {e:.3e} (limit {MC.TOL_Y})")
        assert e < MC.TOL_Y, (name, e)


# ------------------------------------------------------------------------------------------------ 2. kernel
@pytest.mark.parametrize("Mr,C,ldy,ranks,div", MC.KERNEL_SHAPES)
def test_control_mix_kernel_matches_fp64(Mr, C, ldy, ranks, div):
    MC.check_mix_against_fp64(Mr, C, ldy, ranks, div)


def test_control_mix_contract_breaches_are_refused():
    MC.check_contract_breaches()
    y, members, rows_t = MC.mix_inputs(48, 72, 216, (4, 8), 2, seed=5)
    y0 = y.clone()
    with pytest.raises(capi.CloraError):
        K.control_mix_q(y, 68, members, rows_t)                      # the library's refusal reaches the caller
    with pytest.raises(capi.CloraError):
        K.control_mix_q(y, 72, members * 5, rows_t)                  # ten members
    with pytest.raises(capi.CloraError):
        K.control_mix_q(y, 72, members, rows_t // 2)                 # T holds more rows than rows_t says
    with pytest.raises(capi.CloraError):
        K.control_mix_q(y, 72, [(members[0][0], 8, members[0][2], 1.0)], rows_t)    # the rank columns run past T's row
    assert torch.equal(y, y0)


def test_control_mix_wrapper_refuses_cpu_tensors_on_the_product_library():
    y, members, rows_t = MC.mix_inputs(48, 72, 216, (4,), 1)
    old, capi._LIB = capi._LIB, None                                  # the product library, as outside the emulator
    try:
        if not torch.cuda.is_available():
            with pytest.raises(capi.CloraError):
                K.control_mix_q(y, 72, members, rows_t)
    finally:
        capi._LIB = old


# ------------------------------------------------------------------------------------------------ 3. fused site
@pytest.mark.parametrize("arrangement", MC.ARRANGEMENTS)
def test_fused_site_matches_oracle_chain(arrangement):
    MC.check_fused_site(arrangement, "cpu")


# ------------------------------------------------------------------------------------------------ 4. switches
@pytest.mark.parametrize("self_attn", [True, False])
def test_switch_off_is_todays_generic_path(self_attn):
    s = MC.build_site(self_attn, "two_control", "cpu")
    p = s["p_main"]
    with torch.no_grad():
        base = MC.product_site(s)                                     # both switches at their defaults
        for fold_chain in (False, True):
            p.fold_chain, p.fold_control_members = fold_chain, False
            assert p._fold_blocker() is not None and p._needs_generic_path()
            assert torch.equal(MC.product_site(s), base)
            assert "_fold" not in p.__dict__ and "_mix" not in p.__dict__
    assert M.ControlLoRACrossAttnProcessor.fold_control_members is False


@pytest.mark.parametrize("self_attn", [True, False])
def test_ineligible_control_members_report_a_blocker_and_run_generic(self_attn):
    for what in ("v2 main", "concat_hidden member", "post_add member", "autograd on", "member with a chain", "no control states"):
        kw = {}
        if what == "v2 main":
            kw = dict(main="v2")
        elif what == "concat_hidden member":
            kw = dict(member_kw=dict(concat_hidden=True, control_channels=64))
        elif what == "post_add member":
            kw = dict(member_kw=dict(post_add=True))
        s = MC.build_site(self_attn, "control_pre", "cpu", **kw)
        p = s["p_main"]
        grad = what == "autograd on"
        if what == "member with a chain":
            p.pre_loras[0].inject_pre_lora(M.LoRACrossAttnProcessor(64, p.cross_attention_dim, rank=4))
        off = MC.product_site(s, fused=False, grad=grad).detach()
        p.fold_chain = p.fold_control_members = True
        if what == "no control states":
            p.pre_loras[0].control_states = None
        with torch.set_grad_enabled(grad):
            why = p._fold_blocker()
            assert why is not None and p._needs_generic_path(), what
        print(f"MULTI_CONTROL_BLOCKER {what}: {why}")
        if what == "autograd on":
            assert "autograd" in why
        if what == "no control states":
            continue                                                  # (the generic path asserts on the missing states, as the reference)
        on = MC.product_site(s, grad=grad).detach()
        assert torch.equal(on, off), what
        assert "_fold" not in p.__dict__ and "_mix" not in p.__dict__, what


def test_fold_chains_sets_both_switches_and_fold_report_tells_why():
    from tests.e2e_cases import build_product_case
    unet, _, main = build_product_case("v1", "cpu")
    _, member = MC.seeded_control_pair("v1", "cpu", seed=41)
    sites = M.mix_control_loras(unet, main, [member], fold=True)
    assert all(p.fold_chain and p.fold_control_members for p in sites.values())
    rep = main.fold_report()
    assert all(not r["folded"] and "no control states" in r["reason"] and r["control_members"] == 1 for r in rep.values()), rep
    inp = cases.seeded_inputs()
    with torch.no_grad():
        member(inp["guide"][:1].half())
    with torch.no_grad():
        assert all(r["folded"] for r in main.fold_report().values())
    assert all("autograd" in r["reason"] for r in main.fold_report().values())        # autograd is on here
    main.fold_chains(True)                                            # control_members defaults to False
    assert all(p.fold_chain and not p.fold_control_members for p in sites.values())
    with torch.no_grad():
        assert all("not a plain LoRACrossAttnProcessor" in r["reason"] for r in main.fold_report().values())


def test_mix_control_loras_refuses_mixed_versions_and_missing_sites():
    from tests.e2e_cases import build_product_case
    unet, _, main = build_product_case("v1", "cpu")
    _, v2 = MC.seeded_control_pair("v2", "cpu", seed=42)
    with pytest.raises(ValueError, match="version"):
        M.mix_control_loras(unet, main, [v2])
    _, short = MC.seeded_control_pair("v1", "cpu", seed=43)
    del short.lora_layers[3][0]
    with pytest.raises(ValueError, match="no processor for the sites"):
        M.mix_control_loras(unet, main, [short])
    assert not any(p._chain_members() for _, p in main._named_processors()), "a refused mix must not leave members behind"


# ------------------------------------------------------------------------------------------------ 5. staleness
def _fresh(s):
    p = copy.deepcopy(s["p_main"])
    p.__dict__.pop("_fold", None)
    p.__dict__.pop("_mix", None)
    return p


def _out(s, p_main=None):
    with torch.no_grad():
        return MC.product_site(s, p_main)


@pytest.mark.parametrize("self_attn", [True, False])
def test_a_stale_mix_job_is_never_served(self_attn):
    s = MC.build_site(self_attn, "two_control", "cpu")
    p = s["p_main"]
    p.fold_chain = p.fold_control_members = True
    y0 = _out(s)
    mix0, gen0 = p.__dict__["_mix"], p.__dict__["_fold"]["gen"]
    assert torch.equal(y0, _out(s)) and p.__dict__["_mix"] is mix0 and p.__dict__["_fold"]["gen"] == gen0, "an unchanged site rebuilds nothing"
    # new control states on the members: the output moves as the oracle says
    MC.inject_member_controls(s, scale_by=-0.5)
    y1 = _out(s)
    assert p.__dict__["_mix"] is not mix0 and p.__dict__["_fold"]["gen"] == gen0, "new control states rebuild the job, not the fold"
    yo = MC.oracle_site(s)
    assert MC.rel(y1, yo) < MC.TOL_Y and MC.rel(y0, yo) > 2 * MC.TOL_Y, (MC.rel(y1, yo), MC.rel(y0, yo))
    assert torch.equal(y1, _out(s, _fresh(s)))
    # an in-place change of a member's q up matrix: weights refolded, job rebuilt
    mix1 = p.__dict__["_mix"]
    with torch.no_grad():
        p.pre_loras[0].to_q_lora.up.weight.mul_(-1.5)
        s["o_main"].pre_loras[0].to_q_lora.up.weight.mul_(-1.5)
    y2 = _out(s)
    assert p.__dict__["_fold"]["gen"] != gen0 and p.__dict__["_mix"] is not mix1
    assert not torch.equal(y2, y1) and torch.equal(y2, _out(s, _fresh(s)))
    assert MC.rel(y2, MC.oracle_site(s)) < MC.TOL_Y
    # an in-place change of a member's control adapter: the job alone
    with torch.no_grad():
        p.post_loras[0].to_control.up.weight.mul_(0.5)
    y3 = _out(s)
    assert not torch.equal(y3, y2) and torch.equal(y3, _out(s, _fresh(s)))
    # the chain edited
    p.post_loras.clear()
    y4 = _out(s)
    assert not torch.equal(y4, y3) and torch.equal(y4, _out(s, _fresh(s)))
    # another scale
    with torch.no_grad():
        y5 = MC.product_site(s, scale=0.3)
        assert not torch.equal(y5, y4) and torch.equal(y5, MC.product_site(s, _fresh(s), scale=0.3))


def test_a_rebuild_during_graph_capture_raises(monkeypatch):
    s = MC.build_site(True, "control_pre", "cpu")
    p = s["p_main"]
    p.fold_chain = p.fold_control_members = True
    _out(s)
    monkeypatch.setattr(capi.lib(), "require_device", True)           # what the product library reports
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    monkeypatch.setattr(capi, "ptr", lambda t, dtype=None: None if t is None else t.data_ptr())
    monkeypatch.setattr(capi, "stream", lambda: None)
    monkeypatch.setattr(K, "ptr", capi.ptr)
    _out(s)                                                           # nothing stale: a captured step replays what is there
    MC.inject_member_controls(s, scale_by=2.0)
    with pytest.raises(RuntimeError, match="inside a graph capture"):
        _out(s)


# ------------------------------------------------------------------------------------------------ 6. broadcast
@pytest.mark.parametrize("self_attn", [True, False])
def test_batch_one_control_map_equals_the_tiled_map(self_attn):
    one = MC.build_site(self_attn, "two_control", "cpu", ctrl_batch=1)
    tiled = MC.build_site(self_attn, "two_control", "cpu", ctrl_batch=1)
    tiled["member_ctrl"] = {k: v.repeat(tiled["B"], 1, 1, 1) for k, v in tiled["member_ctrl"].items()}
    MC.inject_member_controls(tiled)
    with torch.no_grad():
        ya, yb = MC.product_site(one, fused=True), MC.product_site(tiled, fused=True)
    assert one["p_main"].__dict__["_mix"]["rows_t"] == one["N"] and tiled["p_main"].__dict__["_mix"]["rows_t"] == 2 * one["N"]
    assert torch.equal(ya, yb)
    assert MC.rel(ya, MC.oracle_site(one)) < MC.TOL_Y
    # one member with a map per image beside one with a single map: the single one is tiled once
    mixed = MC.build_site(self_attn, "two_control", "cpu", ctrl_batch=1)
    k0 = next(iter(mixed["member_ctrl"]))
    mixed["member_ctrl"][k0] = mixed["member_ctrl"][k0].repeat(mixed["B"], 1, 1, 1)
    MC.inject_member_controls(mixed)
    with torch.no_grad():
        assert torch.equal(MC.product_site(mixed, fused=True), ya)
    bad = MC.build_site(self_attn, "control_pre", "cpu", B=4, ctrl_batch=2)
    with torch.no_grad(), pytest.raises(ValueError, match="control batch"):
        MC.product_site(bad, fused=True)


# ------------------------------------------------------------------------------------------------ 7. whole small UNet
def test_two_control_unet_matches_oracle_and_adds_one_launch_per_site():
    MC.check_two_control_unet("cpu")


def test_sampler_takes_lists_and_a_list_of_one_is_the_single_call():
    MC.check_sampler_lists("cpu")
