"""GPU tests of the OpenPose kernels and the body network at the real shapes: the cases of tests/openpose_cases.py (derived
elementwise limits against fp64, bit-identical repeat launches) on the 23x23 map the pose app's default gives (M = 529: split-K),
on a batch of 16 (the direct path), the VGG front's 46x46 layer and the 184x184 pool; the network at 2x3x64x88 and 1x3x184x184
layer by layer and end to end against the fp32 / fp16-regime oracles; one whole detector call."""
import numpy as np
import pytest
import torch

from controllora_amd import openpose as OP
from tests import openpose_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("shape", C.CONV7, ids=str)
@pytest.mark.parametrize("relus", [(True,), (False,), (True, False), (False, True)], ids=str)
def test_conv7(shape, relus):
    splits = C.case_conv_act(DEV, *shape, 7, relus=relus)
    if shape[0] == 16:
        assert splits == 1                              # 16 x 9 pixel tiles x 2 channel tiles: the no-split path
    else:
        assert splits > 1


@pytest.mark.parametrize("shape", C.CONV3, ids=str)
def test_conv3(shape):
    C.case_conv_act(DEV, *shape, 3, relus=(True, False))
    C.case_conv_act(DEV, *shape, 3, relus=(True,))


@pytest.mark.parametrize("shape", C.CONV1, ids=str)
def test_conv1(shape):
    C.case_conv_act(DEV, *shape, 1, relus=(False, True))


def test_heads_rejects_pools_and_pack():
    C.case_heads(DEV, 1, 5, 7)
    C.case_heads(DEV, 1, 23, 23)
    C.case_heads(DEV, 16, 23, 23)
    C.case_rejects(DEV)
    for shape in C.POOLS:
        C.case_maxpool(DEV, *shape)
    C.case_pack(DEV)
    C.case_pack(DEV, Cout=38, CinSrc=185, CinDst=192, k=1)


@pytest.fixture(scope="module")
def net():
    return OP.BodyPoseNet.from_pretrained("random:openpose", DEV)


@pytest.mark.parametrize("size", [(2, 64, 88), (1, 184, 184)], ids=str)
def test_network(net, size):
    B, H, W = size
    x = C.net_input(B, H, W).to(DEV)
    paf, heat, acts = net(x, return_activations=True)
    launches = net.launches
    assert paf.shape == (B, 38, H // 8, W // 8) and heat.shape == (B, 19, H // 8, W // 8)
    assert C.check_layerwise(net, x, acts) == (92, 3)
    again = net(x)
    assert torch.equal(again[0], paf) and torch.equal(again[1], heat)
    assert float(heat.min()) >= 0 and float(paf.min()) < 0
    assert 52 <= launches <= 2 * 52 + 3
    print(f"network {size}: {launches} launches per forward")
    C.check_end_to_end(paf, heat, B, H, W)


def test_detector_smoke():
    photo = C.noise_photo()
    det = OP.OpenposeDetector("random:openpose", device=DEV)
    canvas, pose = det(photo)
    assert canvas.shape == photo.shape and canvas.dtype == np.uint8
    assert isinstance(pose["candidate"], list) and isinstance(pose["subset"], list)
    assert all(isinstance(r, list) and len(r) == 4 for r in pose["candidate"]) and all(isinstance(r, list) and len(r) == 20 for r in pose["subset"])
    canvas2, pose2 = det(photo)
    assert np.array_equal(canvas, canvas2) and pose == pose2


def test_pose_app_runs_the_detector_on_the_photo():
    """apps/pose2image.py::process(..., detector=det), the reference's `apply_openpose(resize_image(input_image, detect_resolution))`
    (apps/gradio_pose2image.py:75): the first returned image is the detector's canvas resized with NEAREST"""
    import importlib.util
    import os
    from controllora_amd import models as M
    from controllora_amd.pipeline import ControlLoRAPipeline
    from oracle import cases
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pose2image_det_gpu", os.path.join(root, "apps", "pose2image.py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)
    torch.manual_seed(0)
    pipe = ControlLoRAPipeline.from_pretrained("random:small", M.ControlLoRA(**cases.SMALL_CLORA_V1), DEV)
    det = OP.OpenposeDetector("random:openpose", device=DEV)
    photo = C.noise_photo(96, 128)
    out = app.process(pipe, photo, "a man", "best quality", "lowres", 2, 64, 128, 2, 5.0, 7, 0.0, detector=det)
    want, _ = det(app.resize_image(app.hwc3(photo), 128))
    H, W = app.resize_image(photo, 64).shape[:2]
    assert len(out) == 3 and all(o.shape == (H, W, 3) and o.dtype == np.uint8 for o in out)
    assert np.array_equal(out[0], app.nearest_resize(want, W, H))
