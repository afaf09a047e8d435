"""CPU tests of the host half of the OpenPose detector (controllora_amd/openpose.py): post-processing on planted maps, the cubic
resize matrices, drawing, the layer table and both state-dict layouts; and, where the reference tree is present, the plain-torch
restatement of tests/openpose_cases.py against `annotator/openpose/model.py::bodypose_model` run in place with the same weights."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from controllora_amd import openpose as OP
from tests import openpose_cases as C

REFERENCE = "/root/reference"


# ---------------------------------------------------------------- post-processing
def test_planted_skeletons_are_found_exactly():
    people = C.planted_people()
    heat, paf = C.planted_maps(people)
    assert heat.shape == (96, 128, 19) and paf.shape == (96, 128, 38)
    for person in people:                                   # the generator's own contract: 16 px from every border
        for x, y in person.values():
            assert 16 <= x <= 128 - 16 and 16 <= y <= 96 - 16
    candidate, subset = OP.postprocess(heat, paf)
    planted = sorted((i, y, x) for person in people for i, (x, y) in person.items())
    assert candidate.shape == (len(planted), 4)
    assert [(int(c[0]), int(c[1])) for c in candidate] == [(x, y) for _, y, x in planted]          # by part, then row-major: exactly the planted pixels
    assert np.array_equal(candidate[:, 3], np.arange(len(planted))) and np.all(candidate[:, 2] == 1.0)
    assert subset.shape == (2, 20)                          # the three-joint stub is deleted by the `< 4 parts` rule
    rows = sorted(subset.tolist(), key=lambda r: candidate[int(r[1])][0])                            # by the neck's x
    for n, row in enumerate(rows):
        for i in range(18):
            if (n, i) == C.MISSING:
                assert row[i] == -1
            else:
                assert tuple(candidate[int(row[i])][:2]) == people[n][i], (n, i)
    assert [r[19] for r in rows] == [18, 17]
    assert all(r[18] / r[19] > 0.4 for r in rows)


def test_stub_alone_is_deleted_and_empty_maps_give_empty_results():
    heat, paf = C.planted_maps([dict(C.THIRD)])
    candidate, subset = OP.postprocess(heat, paf)
    assert candidate.shape == (3, 4) and subset.shape == (0, 20)
    candidate, subset = OP.postprocess(np.zeros((32, 40, 19)), np.zeros((32, 40, 38)))
    assert candidate.shape == (0, 4) and subset.shape == (0, 20)


# ---------------------------------------------------------------- resizes
def test_resize_matrices():
    for n_src, n_dst, inv in ((23, 184, 1 / 8), (184, 512, None), (96, 46, None), (7, 7, None), (50, 23, 50 / 23.3)):
        R = OP.cubic_matrix(n_src, n_dst, inv)
        assert R.shape == (n_dst, n_src) and np.allclose(R.sum(1), 1.0, atol=1e-12)
    assert np.array_equal(OP.cubic_matrix(9, 9), np.eye(9))                                           # scale 1 is the identity
    # a 1-D impulse, halved: destination d samples 2 d + 0.5, phase 0.5, closed-form Keys taps for a = -0.75
    R = OP.cubic_matrix(16, 8)
    assert np.allclose(R[3, 5:9], [-0.09375, 0.59375, 0.59375, -0.09375], atol=1e-15) and np.count_nonzero(R[3]) == 4
    assert np.allclose(OP.cubic_taps(np.array(0.5)), [-0.09375, 0.59375, 0.59375, -0.09375])
    assert np.allclose(R @ np.eye(16)[:, 7], [0, 0, 0, 0.59375, -0.09375, 0, 0, 0])                 # the impulse at 7: d = 3 reads 5 .. 8, d = 4 reads 7 .. 10
    # replicated border: the first destination pixel of a x2 upscale reads source -1 as source 0
    U = OP.cubic_matrix(4, 8, 0.5)
    t = OP.cubic_taps(np.array(0.75))                                                              # d = 0 samples -0.25: taps at -2, -1, 0, 1
    assert np.allclose(U[0], [t[0] + t[1] + t[2], t[3], 0, 0])
    # x8, crop the pad, resize to the photo: a constant map stays the constant
    My, Mx = OP.map_resize_matrices(23, 32, 3, 5, 100, 140)
    assert My.shape == (100, 23) and Mx.shape == (140, 32)
    out = OP.resize_cubic(np.full((23, 32, 2), 0.37), My, Mx)
    assert out.shape == (100, 140, 2) and np.allclose(out, 0.37, atol=1e-12)
    img = np.arange(5 * 6 * 3, dtype=np.float64).reshape(5, 6, 3)
    assert np.allclose(OP.resize_cubic(img, OP.cubic_matrix(5, 5), OP.cubic_matrix(6, 6)), img)
    assert OP.to_uint8(np.array([-3.0, 0.5, 1.5, 254.5, 300.0])).tolist() == [0, 0, 2, 254, 255]


# ---------------------------------------------------------------- drawing
def test_drawing():
    cand = np.array([[30, 30, 1.0, 0], [30, 60, 1.0, 1]], np.float64)                              # nose, neck: limb 12 is [2, 1]
    subset = -np.ones((1, 20))
    subset[0, 0], subset[0, 1], subset[0, 19] = 0, 1, 2
    canvas = np.zeros((90, 70, 3), np.uint8)
    out = OP.draw_bodypose(canvas, cand, subset)
    assert out.shape == canvas.shape and out.dtype == np.uint8 and not canvas.any()                # the input is not drawn on
    limb = np.array(OP.COLORS[12])
    assert np.array_equal(out[45, 30], np.rint(0.6 * limb).astype(np.uint8))                       # the centre of an isolated limb
    # a pixel inside the nose's disc AND inside the limb: the disc's colour blended once with the limb's
    disc0 = np.array(OP.COLORS[0], np.float64)
    assert np.array_equal(out[33, 31], np.rint(0.4 * disc0 + 0.6 * limb).astype(np.uint8))
    assert out[28, 30].tolist() == OP.COLORS[0]                                                    # inside the disc, outside the limb
    assert not out[5, 5].any() and not out[80, 60].any()                                          # untouched pixels stay 0
    # discs alone (no limb: the two joints are not a limb pair): interior pixels have their colours
    subset2 = -np.ones((1, 20))
    subset2[0, 4], subset2[0, 10], subset2[0, 19] = 0, 1, 2
    out2 = OP.draw_bodypose(np.zeros((90, 70, 3), np.uint8), cand, subset2)
    assert out2[30, 30].tolist() == OP.COLORS[4] and out2[60, 30].tolist() == OP.COLORS[10] and out2[32, 32].tolist() == OP.COLORS[4]
    assert not out2[45, 30].any()
    # two crossing limbs blend in drawing order: limb 0 ([2, 3] neck - r.shoulder) first, limb 1 ([2, 6] neck - l.shoulder) over it
    cand3 = np.array([[20, 40, 1.0, 0], [60, 40, 1.0, 1], [40, 20, 1.0, 2], [40, 60, 1.0, 3]], np.float64)
    a, b = -np.ones(20), -np.ones(20)
    a[1], a[2], b[1], b[5] = 0, 1, 2, 3
    out3 = OP.draw_bodypose(np.zeros((80, 80, 3), np.uint8), cand3, np.stack([a, b]))
    first = np.rint(0.6 * np.array(OP.COLORS[0], np.float64))
    want = np.rint(0.4 * first + 0.6 * np.array(OP.COLORS[1], np.float64)).astype(np.uint8)
    assert np.array_equal(out3[40, 40], want)
    assert np.array_equal(out3[40, 30], first.astype(np.uint8))                                    # limb 0 alone: a later blend leaves it (0.4 c + 0.6 c)
    assert OP.add_weighted(np.array([5], np.uint8), 0.5, np.array([0], np.uint8), 0.5).tolist() == [2]      # 2.5 -> 2: nearest even
    assert OP.add_weighted(np.array([255], np.uint8), 1.0, np.array([255], np.uint8), 1.0).tolist() == [255]


# ---------------------------------------------------------------- the layer table and the restatement
def test_layer_table_and_relu_quirk():
    table = OP.layer_table()
    convs = [L for L in table if L["ksize"]]
    assert len(convs) == 92 and len(table) - len(convs) == 3
    assert sum(1 for L in convs if L["ksize"] == 7) == 50 and sum(1 for L in convs if L["Cin"] == 185) == 10
    no_relu = {L["name"] for L in convs if not L["relu"]}
    assert no_relu == {"conv5_5_CPM_L1", "conv5_5_CPM_L2"} | {f"Mconv7_stage{s}_L{b}" for s in range(2, 7) for b in (1, 2)} - {"Mconv7_stage6_L2"}
    perm = OP.concat_permutation()
    assert len(perm) == 192 and sorted(p for p in perm if p >= 0) == list(range(185)) and perm[0] == 57 and perm[128] == 0 and perm[166] == 38
    sd = OP.random_state_dict(0)
    ref = C.RefBodyPose(sd)
    x = C.net_input(1, 16, 24)
    with torch.no_grad():
        paf, heat = ref.forward(x, "fp32")
    assert paf.shape == (1, 38, 2, 3) and heat.shape == (1, 19, 2, 3)
    assert float(heat.min()) >= 0 and float(paf.min()) < 0                                        # Mconv7_stage6_L2 is clipped at 0, L1 is not
    assert abs(float(sd["Mconv3_stage4_L2.weight"].std()) - (2.0 / (128 * 49)) ** 0.5) < 2e-4 and not sd["conv1_1.bias"].any()


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference tree is not present")
def test_restatement_equals_the_reference_model_in_place():
    spec = importlib.util.spec_from_file_location("ref_openpose_model", os.path.join(REFERENCE, "annotator", "openpose", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    model = mod.bodypose_model().eval()
    sd = OP.random_state_dict(0)
    ref = C.RefBodyPose(sd)
    assert sorted(ref.state_dict()) == sorted(model.state_dict())                                  # the keys, exactly
    assert all(ref.state_dict()[k].shape == v.shape for k, v in model.state_dict().items())
    model.load_state_dict(ref.state_dict())
    x = C.net_input(1, 40, 56).float()
    with torch.no_grad():
        want = model(x)
        got = ref.forward(x, "fp32")
    for g, w in zip(got, want):
        assert g.shape == w.shape and float((g - w).norm() / w.norm()) <= 1e-6
    assert float(want[1].min()) >= 0 and float(want[0].min()) < 0                                  # the quirk is the reference's own


def test_both_key_layouts_load(monkeypatch):
    """bare names (the converted Caffe file) and module-prefixed names give the same network; packing is stubbed out (it is a kernel
    launch, covered on the emulator): this test is about the keys"""
    from controllora_amd import kernels as K
    monkeypatch.setattr(K, "conv_act_pack", lambda w, Cin=None, perm=None: torch.zeros(1))
    bare = OP.random_state_dict(1)
    pref = C.RefBodyPose(bare).state_dict()
    assert "model0.conv1_1.weight" in pref and "model3_2.Mconv4_stage3_L2.bias" in pref
    a, b = OP.BodyPoseNet(bare, "cpu"), OP.BodyPoseNet(pref, "cpu")
    assert sorted(a.state_dict()) == sorted(b.state_dict()) == sorted(bare)
    assert all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in bare)
    wrong = dict(pref)
    wrong["model1_1.conv1_1.weight"] = wrong.pop("model0.conv1_1.weight")
    with pytest.raises(KeyError):
        OP.BodyPoseNet(wrong, "cpu")
    short = dict(bare)
    short.pop("Mconv7_stage6_L2.bias")
    with pytest.raises(KeyError):
        OP.BodyPoseNet(short, "cpu")
