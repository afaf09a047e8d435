"""CPU tests of chained version-2 ControlLoRAs on the emulated kernels: the control-chain kernel (clora_control_chain_f16) against
fp64, what the site cases can see, the fused v2 site against the oracle chain, the recorded reference outputs through the fused path,
blockers, stale jobs, and a whole small UNet steered by two v2 control models."""
import pytest
import torch

from controllora_amd import capi, kernels as K, models as M
from tests import multi_control_cases as MC
from tests import multi_control_v2_cases as V2
from tests.emu_fixture import use_emulator

f16, f32 = torch.float16, torch.float32


@pytest.fixture(autouse=True)
def _emu():
    with use_emulator():
        yield


# ------------------------------------------------------------------------------------------------ 1. kernel
@pytest.mark.parametrize("Mr,C,ranks,div", V2.KERNEL_SHAPES)
def test_control_chain_kernel_matches_fp64(Mr, C, ranks, div):
    V2.check_chain_against_fp64(Mr, C, ranks, div)


def test_control_chain_kernel_in_place_and_with_pitches_and_offsets():
    V2.check_chain_against_fp64(75, 72, (4, 12, 16), 3, in_place=True)
    V2.check_chain_against_fp64(128, 320, (4, 4), 1, padded=True)           # ldh, ldy, ldd > C, Tc at a column offset
    V2.check_chain_against_fp64(3 * 128 + 21, 72, (8, 8), 3, in_place=True, padded=True)


def test_control_chain_kernel_past_the_sd_widths():
    """columns beyond five words per lane of half a wave: the full-wave row layout, up to the documented limit of 2560 columns"""
    V2.check_chain_against_fp64(16, 1288, (4, 4), 1)
    V2.check_chain_against_fp64(8, 2560, (4, 8), 1)
    H, members, G, rows_t = V2.chain_inputs(8, 2568, (4,), 1)
    with pytest.raises(capi.CloraError):
        K.control_chain(H, torch.empty_like(H), members, None, 0.7, rows_t)


def test_control_chain_kernel_ranks_off_the_four_rank_batches():
    """the kernel walks the stacked ranks four at a time: totals that end inside a batch, members that straddle one"""
    for ranks, div in (((3, 5), 1), ((1, 2), 2), ((5,), 1), ((7, 6, 1), 1), ((16, 9), 2)):
        V2.check_chain_against_fp64(40, 72, ranks, div)


def test_control_chain_contract_breaches_are_refused():
    V2.check_contract_breaches()
    H, members, G, rows_t = V2.chain_inputs(48, 72, (4, 8), 2, seed=5)
    y = torch.zeros(48, 72, dtype=f16)
    with pytest.raises(capi.CloraError):
        K.control_chain(H, y, members * 5, G, 0.7, rows_t)                   # ten members
    with pytest.raises(capi.CloraError):
        K.control_chain(H, y, members, G, 0.7, rows_t // 2)                  # Tc holds more rows than rows_t says
    with pytest.raises(capi.CloraError):
        K.control_chain(H, y, members, None, 0.7, rows_t)                    # two members without G
    with pytest.raises(capi.CloraError):
        K.control_chain(H, y, [(members[0][0], members[0][1], members[0][2], 8)], None, 0.7, rows_t)   # the rank columns run past Tc's row
    assert not bool(y.any())


def test_control_chain_wrapper_refuses_cpu_tensors_on_the_product_library():
    H, members, G, rows_t = V2.chain_inputs(48, 72, (4,), 1)
    old, capi._LIB = capi._LIB, None                                  # the product library, as outside the emulator
    try:
        if not torch.cuda.is_available():
            with pytest.raises(capi.CloraError):
                K.control_chain(H, torch.empty_like(H), members, None, 0.7, rows_t)
    finally:
        capi._LIB = old


# ------------------------------------------------------------------------------------------------ 2. + 3. fused site
@pytest.mark.parametrize("arrangement", V2.ARRANGEMENTS)
def test_site_cases_can_see_coupling_control_maps_and_order(arrangement):
    """the oracle alone: the chain without coupling, without the members' maps, and in another order is far from the chain"""
    for self_attn in (True, False):
        V2.check_site_can_see(V2.build_site(self_attn, arrangement, "cpu"), f"{arrangement}/{'self' if self_attn else 'cross'}")


@pytest.mark.parametrize("arrangement", V2.ARRANGEMENTS)
def test_fused_v2_site_matches_oracle_chain(arrangement):
    V2.check_fused_site(arrangement, "cpu")


def test_batch_one_member_maps_are_tiled_once():
    s = V2.build_site(True, "member_batch_1", "cpu")
    with torch.no_grad():
        ya = MC.product_site(s, fused=True)
    st = s["p_main"].__dict__["_chain"]
    assert st["rows_t"] == s["B"] * s["N"] and all(m[2].shape[0] == st["rows_t"] for m in st["in"][0] + st["out"][0])
    tiled = V2.build_site(True, "member_batch_1", "cpu")
    tiled["member_ctrl"] = {k: v.repeat(tiled["B"], 1, 1, 1) for k, v in tiled["member_ctrl"].items()}
    MC.inject_member_controls(tiled)
    with torch.no_grad():
        assert torch.equal(MC.product_site(tiled, fused=True), ya)


# ------------------------------------------------------------------------------------------------ 4. records
def test_fused_path_reproduces_the_v2_records():
    records = MC.load_records()
    names = [n for n in sorted(records) if n.split(":")[0] in V2.V2_RECORD_CASES]
    assert len(names) == 8, names                                     # two cases x self / cross x control batch 1 / 2
    for name in names:
        y, ya, _ = V2.replay_record_fused(name, records[name])
        e = V2.rel(y, ya)
        print(f"MULTI_CONTROL_V2_RECORD {name}: fused path {e:.3e} (limit {V2.TOL_Y})")
        assert e < V2.TOL_Y, (name, e)


# ------------------------------------------------------------------------------------------------ 5. blockers, staleness, capture
@pytest.mark.parametrize("self_attn", [True, False])
@pytest.mark.parametrize("what", V2.BLOCKERS)
def test_ineligible_v2_chains_report_a_blocker_and_run_generic(what, self_attn):
    V2.check_blocker(what, self_attn, "cpu")


def test_a_v2_member_on_a_v1_main_reports_a_blocker():
    s = MC.build_site(True, "control_pre", "cpu")
    p = s["p_main"]
    p.inject_post_lora(M.ControlLoRACrossAttnProcessorV2(64, None, rank=4, control_channels=32))
    p.fold_chain = p.fold_control_members = True
    with torch.no_grad():
        assert "not version 2" in p._fold_blocker()


@pytest.mark.parametrize("self_attn", [True, False])
def test_a_stale_chain_job_is_never_served(self_attn):
    V2.check_staleness(self_attn, "cpu")


def test_a_rebuild_during_graph_capture_raises(monkeypatch):
    s = V2.build_site(True, "member_pre", "cpu")
    p = s["p_main"]
    p.fold_chain = p.fold_control_members = True
    with torch.no_grad():
        MC.product_site(s)
    monkeypatch.setattr(capi.lib(), "require_device", True)           # what the product library reports
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    monkeypatch.setattr(capi, "ptr", lambda t, dtype=None: None if t is None else t.data_ptr())
    monkeypatch.setattr(capi, "stream", lambda: None)
    monkeypatch.setattr(K, "ptr", capi.ptr)
    V2.call_site(s)                                                   # nothing stale: a captured step replays what is there
    MC.inject_member_controls(s, scale_by=2.0)
    with pytest.raises(RuntimeError, match="inside a graph capture"):
        V2.call_site(s)


def test_fold_chains_drops_the_chain_job_and_fold_report_names_the_reasons():
    from tests.e2e_cases import build_product_case
    unet, _, main = build_product_case("v2", "cpu")
    _, member = MC.seeded_control_pair("v2", "cpu", seed=41)
    sites = M.mix_control_loras(unet, main, [member], fold=True)
    assert all(p.fold_chain and p.fold_control_members for p in sites.values())
    with torch.no_grad():
        rep = main.fold_report()
    assert all(not r["folded"] and "no control states" in r["reason"] and r["control_members"] == 1 for r in rep.values()), rep
    inp = MC.small_inputs()
    MC.forward(unet, [main, member], inp, [inp["guide"], -inp["guide"]], "cpu")
    with torch.no_grad():
        assert all(r["folded"] for r in main.fold_report().values())
    assert all("autograd" in r["reason"] for r in main.fold_report().values())        # autograd is on here
    assert all(V2.states(p) == ["_chain", "_fold"] for p in sites.values())
    main.fold_chains(True)                                            # control_members defaults to False
    assert all(V2.states(p) == ["_fold"] for p in sites.values())
    with torch.no_grad():
        assert all("not a plain LoRACrossAttnProcessor" in r["reason"] for r in main.fold_report().values())
    main.fold_chains(False)
    assert all(V2.states(p) == [] for p in sites.values())


# ------------------------------------------------------------------------------------------------ 6. whole small UNet
def test_two_v2_control_unet_matches_oracle_with_two_chain_launches_per_site():
    V2.check_two_control_unet("cpu")
