"""CPU tests of the OpenPose kernels (controllora_amd/csrc/clora_pose.hip) and of the body network on the host fiber emulator: the
cases of tests/openpose_cases.py at their smallest shapes -- a map smaller than the 7x7 halo, ragged 8x8 tiles with a batch seam, the
padded image layer, the 1x1 heads storing into the 192-channel stage buffer -- every one on the split-K path its size takes (the
emulator reports 256 CUs like an MI355X), plus the whole network at 1x3x40x56 layer by layer and end to end."""
import numpy as np
import pytest
import torch

from controllora_amd import capi, kernels as K, openpose as OP
from tests import openpose_cases as C
from tests.emu_fixture import use_emulator


@pytest.mark.parametrize("shape", C.CONV7[:2], ids=str)
@pytest.mark.parametrize("relus", [(True,), (False,), (True, False), (False, True)], ids=str)
def test_conv7(shape, relus):
    with use_emulator():
        splits = C.case_conv_act("cpu", *shape, 7, relus=relus)
    assert splits > 1                                   # few tiles: K is split, the slabs and the finish pass run


def test_conv3_conv1_and_heads():
    with use_emulator():
        C.case_conv_act("cpu", *C.CONV3[0], 3, relus=(True,))
        C.case_conv_act("cpu", *C.CONV3[1], 3, relus=(True, False))
        C.case_conv_act("cpu", *C.CONV1[0], 1, relus=(True, False))
        C.case_heads("cpu", 1, 5, 7)
        C.case_heads("cpu", 2, 13, 9)


def test_direct_path_on_the_emulator():
    """enough tiles for one launch without slabs: 5 x 7 pixel tiles x 2 channel tiles x 2 jobs x batch 2 = 280 >= 256"""
    with use_emulator():
        assert C.case_conv_act("cpu", 2, 40, 56, 8, 70, 3, relus=(True, False), seed=9) == 1


def test_rejects_pool_and_pack():
    with use_emulator():
        C.case_rejects("cpu")
        C.case_maxpool("cpu", *C.POOLS[0])
        C.case_pack("cpu")
        C.case_pack("cpu", Cout=38, CinSrc=185, CinDst=192, k=1)


def test_wrappers_refuse_cpu_tensors_without_the_emulator():
    if not torch.cuda.is_available():                   # product library + CPU tensors -> loud error, not a fallback
        with pytest.raises(capi.CloraError):
            K.maxpool2x2(torch.zeros(1, 2, 2, 8, dtype=torch.float16))
        with pytest.raises(capi.CloraError):
            OP.BodyPoseNet.from_pretrained("random:openpose", "cpu")


@pytest.fixture(scope="module")
def small_net_run():
    with use_emulator():
        net = OP.BodyPoseNet.from_pretrained("random:openpose", "cpu")
        x = C.net_input(1, 40, 56)
        paf, heat, acts = net(x, return_activations=True)
        launches = net.launches
        again = net(x)
    return net, x, paf, heat, acts, launches, again


def test_network_layerwise(small_net_run):
    net, x, paf, heat, acts, launches, again = small_net_run
    assert paf.shape == (1, 38, 5, 7) and heat.shape == (1, 19, 5, 7) and paf.dtype == heat.dtype == torch.float16
    assert C.check_layerwise(net, x, acts) == (92, 3)
    assert torch.equal(again[0], paf) and torch.equal(again[1], heat)                   # a second forward: the same bits
    assert float(heat.min()) >= 0 and float(paf.min()) < 0                              # the Mconv7_stage6_L2 ReLU quirk; L1 has none
    assert 52 <= launches <= 2 * 52 + 3              # one launch per layer pair (+ a finish pass where K is split) + 3 pools


def test_network_end_to_end(small_net_run):
    _, _, paf, heat, *_ = small_net_run
    C.check_end_to_end(paf, heat, 1, 40, 56)


def test_network_rejects_bad_inputs():
    with use_emulator():
        net = OP.BodyPoseNet(device="cpu")
        with pytest.raises(KeyError):
            net.load_state_dict({"conv1_1.weight": torch.zeros(64, 3, 3, 3)})
        with pytest.raises(ValueError):
            net.forward(torch.zeros(1, 3, 40, 52, dtype=torch.float16))


def test_detector_smoke_and_the_pose_app():
    """OpenposeDetector on a 64x88 noise photo (box size 64 instead of 368: the emulator runs one fiber per GPU thread), then the same
    detector through apps/pose2image.py::process and the small pipeline of tests/e2e_cases.py: the first returned image is the
    detector's canvas resized with NEAREST, and it is what the control tensor was made from"""
    import importlib.util
    import os
    from controllora_amd import models as M
    from controllora_amd.pipeline import ControlLoRAPipeline
    from oracle import cases
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pose2image_det", os.path.join(root, "apps", "pose2image.py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)
    photo = C.noise_photo()
    with use_emulator():
        det = OP.OpenposeDetector("random:openpose", device="cpu", boxsize=64)
        canvas, pose = det(photo)
        assert canvas.shape == photo.shape and canvas.dtype == np.uint8
        assert isinstance(pose["candidate"], list) and isinstance(pose["subset"], list)
        assert all(isinstance(r, list) and len(r) == 4 for r in pose["candidate"]) and all(isinstance(r, list) and len(r) == 20 for r in pose["subset"])
        with pytest.raises(NotImplementedError):
            det(photo, hand=True)
        torch.manual_seed(0)
        clora = M.ControlLoRA(**cases.SMALL_CLORA_V1)
        pipe = ControlLoRAPipeline.from_pretrained("random:small", clora, "cpu")
        seen = {}
        orig = pipe.__class__.__call__

        def spy(self, prompt, control, **kw):
            seen.update(control=control.clone())
            return orig(self, prompt, control, **kw)
        pipe.__class__.__call__ = spy
        try:
            out = app.process(pipe, photo, "a man", "best quality", "lowres", 1, 64, 64, 1, 5.0, 7, 0.0, detector=det)
        finally:
            pipe.__class__.__call__ = orig
        want_canvas, _ = det(app.resize_image(app.hwc3(photo), 64))
    H, W = app.resize_image(photo, 64).shape[:2]
    assert len(out) == 2 and np.array_equal(out[0], app.nearest_resize(want_canvas, W, H))
    assert torch.equal(seen["control"], torch.from_numpy(out[0][..., ::-1].copy().transpose(2, 0, 1)).float()[None] / 127.5 - 1.0)
    with pytest.raises(ValueError):
        app.process(pipe, photo, "a man", "", "", 1, 64, 64, 1, 5.0, 7, 0.0, pose_map=photo, detector=det)
