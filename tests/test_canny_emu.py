"""CPU tests of the device Canny detector (controllora_amd/csrc/clora_canny.hip) on the host fiber emulator, against the numpy
detector `controllora_amd.process.canny`, which is the specification.  The contract has two stages (INTEGRATION.md "Canny"):

1. classify: the class map equals numpy's at every pixel that is not ambiguous (tests/canny_cases.py: `mag >= low` and the float64
   angle within 1e-3 degrees of a sector boundary, where numpy's fp32 atan2 is rounding noise); at most 2e-4 of an image's pixels
   may be ambiguous, asserted before every comparison.  The inputs of this file have an EMPTY ambiguous mask (asserted), so the
   class maps are compared for plain equality.
2. hysteresis: given the same class map, bit for bit numpy's loop.  No exceptions.
3. composition: `kernels.canny(img)` == numpy hysteresis of the device's own class map, bit for bit.

The emulator runs one fiber per GPU thread: images stay around 64x96."""
import numpy as np
import pytest
import torch

from controllora_amd import capi, data, kernels as K, process as P
from tests import canny_cases as CC
from tests.emu_fixture import use_emulator

# (seed, H, W, C, sigma): RGB and grey, sizes that are no multiple of the 64x16 / 64x32 tiles, 1xN and Nx1 strips
IMAGES = [(0, 64, 96, 3, 0.0), (1, 37, 53, 3, 1.5), (2, 40, 150, 1, 2.0), (3, 1, 70, 3, 0.0), (4, 70, 1, 1, 0.0), (5, 33, 65, 1, 0.0),
          (6, 17, 129, 3, 1.0)]


def _image(case):
    seed, H, W, C, sigma = case
    lo, hi = CC.thresholds(seed, 1)
    return CC.noise_image(seed, H, W, C, sigma), float(lo[0]), float(hi[0])


def _batch(img):
    t = torch.from_numpy(img)
    return (t[None] if img.ndim == 3 else t[None, :, :, None]).contiguous()


def _thr(*v):
    return torch.tensor(v, dtype=torch.float32)


def hysteresis_maps():
    """hand-made class maps; tiles of the hysteresis kernel are 64 wide and 32 tall"""
    maps = {"snake": CC.snake(40, 150, True), "snake_without_strong": CC.snake(40, 150, False),
            "snake_tall": np.ascontiguousarray(CC.snake(140, 70, True).T)}            # vertical runs: crosses the horizontal tile borders
    d = np.zeros((70, 140), np.uint8)                                                  # weak diagonal chain: 8-connectivity only
    i = np.arange(70)
    d[i, i + 30] = 1
    d[0, 30] = 2
    maps["diagonal"] = d
    a = np.zeros((50, 100), np.uint8)                                                  # anti-diagonal chain, strong at its far end
    a[np.arange(50), 99 - np.arange(50) - 10] = 1
    a[49, 40] = 2
    maps["anti_diagonal"] = a
    two = np.zeros((48, 130), np.uint8)                                                # two weak components, one touches a strong pixel
    two[10, 5:125] = 1
    two[11, 125] = 2
    two[30, 5:125] = 1
    maps["two_components"] = two
    c = np.zeros((66, 130), np.uint8)                                                  # strong pixels on the image border / in tile corners
    c[0, :] = 1
    c[:, 0] = 1
    c[65, :] = 1
    c[:, 129] = 1
    c[0, 0] = c[65, 129] = 2
    c[31:34, 63:66] = 1                                                                # the corner where four tiles meet
    c[32, 64] = 2
    c[20:31, 63] = 1
    c[40, 70:90] = 1                                                                   # isolated weak run: stays dark
    maps["borders_and_corners"] = c
    maps["all_weak"] = np.ones((35, 70), np.uint8)
    maps["all_strong"] = np.full((35, 70), 2, np.uint8)
    maps["all_weak_one_strong"] = maps["all_weak"].copy()
    maps["all_weak_one_strong"][34, 69] = 2
    maps["empty"] = np.zeros((5, 9), np.uint8)
    return maps


def test_restatement_equals_the_shipped_detector():
    """pure numpy: classify_np + hysteresis_np ARE process.canny on every image used below, and the flood fill used for long
    chains on the GPU is the loop's fixed point on every small map"""
    for case in IMAGES:
        img, lo, hi = _image(case)
        assert np.array_equal(CC.hysteresis_np(CC.classify_np(img, lo, hi)), P.canny(img, lo, hi)), case
        assert np.array_equal(CC.hysteresis_np(CC.classify_np(img, hi, hi)), P.canny(img, hi, hi)), case
        cls = CC.classify_np(img, lo, hi)
        assert np.array_equal(CC.hysteresis_flood(cls), CC.hysteresis_np(cls))
    for name, m in hysteresis_maps().items():
        assert np.array_equal(CC.hysteresis_flood(m), CC.hysteresis_np(m)), name
    flat = np.full((20, 30, 3), 77, np.uint8)
    assert not P.canny(flat, 1, 2).any() and not CC.classify_np(flat, 1, 2).any()


@pytest.mark.parametrize("case", IMAGES, ids=lambda c: f"{c[1]}x{c[2]}x{c[3]}")
def test_classify_equals_numpy(case):
    img, lo, hi = _image(case)
    assert not CC.ambiguous_np(img, lo).any(), "pick another seed: this file compares class maps for plain equality"
    with use_emulator():
        got = K.canny_classify(_batch(img), _thr(lo), _thr(hi))[0].numpy()
        same = K.canny_classify(_batch(img), _thr(hi), _thr(hi))[0].numpy()              # low == high: no weak class
    assert CC.check_classify(got, img, lo, hi) == 0
    assert np.array_equal(got, CC.classify_np(img, lo, hi))
    assert len(np.unique(got)) == 3 or min(img.shape[:2]) == 1                           # the input exercises all three classes
    assert np.array_equal(same, CC.classify_np(img, hi, hi)) and not (same == 1).any()


@pytest.mark.parametrize("C", [3, 1])
def test_classify_batch_with_thresholds_per_image(C):
    imgs = [CC.noise_image(20 + i, 45, 83, C, sigma) for i, sigma in enumerate((0.0, 1.0, 2.0))]
    lo, hi = CC.thresholds(7, 3)
    assert len({(a, b) for a, b in zip(lo, hi)}) == 3
    for img, l in zip(imgs, lo):
        assert not CC.ambiguous_np(img, l).any()
    x = torch.from_numpy(np.stack(imgs))
    with use_emulator():
        got = K.canny_classify(x if C == 3 else x[..., None].contiguous(), torch.from_numpy(lo), torch.from_numpy(hi)).numpy()
    for i, img in enumerate(imgs):
        assert np.array_equal(got[i], CC.classify_np(img, lo[i], hi[i])), i


def test_classify_flat_image_is_all_class_zero_and_thresholds_swap_like_cv2():
    flat = np.full((40, 70, 3), 200, np.uint8)
    img, lo, hi = _image(IMAGES[0])
    with use_emulator():
        assert not K.canny_classify(_batch(flat), _thr(1.0), _thr(1.0)).any()
        swapped = K.canny_classify(_batch(img), _thr(hi), _thr(lo))[0].numpy()
    assert np.array_equal(swapped, CC.classify_np(img, lo, hi))


@pytest.mark.parametrize("name", sorted(hysteresis_maps()))
def test_hysteresis_equals_the_numpy_loop(name):
    m = hysteresis_maps()[name]
    want = CC.hysteresis_np(m)
    stats = {}
    with use_emulator():
        got = K.canny_hysteresis(torch.from_numpy(m)[None], stats=stats)[0].numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want), name
    if name in ("snake", "snake_tall", "all_weak", "all_weak_one_strong", "all_strong"):
        assert np.array_equal(got > 0, m >= 1) if name != "all_weak" else not got.any()  # all of it lights up / nothing does
    if name == "snake_without_strong":
        assert not got.any() and stats["groups"] == 1
    if name in ("diagonal", "anti_diagonal"):
        assert (got > 0).sum() == (m >= 1).sum()
    if name == "two_components":
        assert got[10, 5:125].all() and not got[30].any()
    assert stats["passes"] >= 1 and stats["launches"] == stats["passes"] + stats["groups"] + 2


def test_hysteresis_batch_keeps_images_apart():
    maps = hysteresis_maps()
    a, b = maps["snake"], maps["snake_without_strong"]
    with use_emulator():
        got = K.canny_hysteresis(torch.from_numpy(np.stack([a, b, a]))).numpy()
    assert np.array_equal(got[0], CC.hysteresis_np(a)) and not got[1].any() and np.array_equal(got[2], got[0])


def test_hysteresis_pass_bound_is_an_error_not_a_loop():
    """more passes than pixels cannot happen for a monotone growth: the export refuses instead of looping"""
    from tests.emu_fixture import emu_lib
    L = emu_lib()
    st = torch.ones(4, 4, dtype=torch.uint8)
    fl = torch.zeros(capi.CANNY_MAX_GROUP + 1, dtype=torch.int32)
    f = L.cdll.clora_canny_hysteresis_u8
    assert f(st.data_ptr(), fl.data_ptr(), 16, 4, 1, 4, 4, None) == capi.OK
    assert f(st.data_ptr(), fl.data_ptr(), 17, 4, 1, 4, 4, None) == capi.ERR_ARG
    assert f(st.data_ptr(), fl.data_ptr(), 0, capi.CANNY_MAX_GROUP + 1, 1, 4, 4, None) == capi.ERR_ARG
    assert f(st.data_ptr(), fl.data_ptr(), 0, 0, 1, 4, 4, None) == capi.ERR_ARG
    assert L.cdll.clora_canny_classify_u8(st.data_ptr(), fl.data_ptr(), fl.data_ptr(), st.data_ptr(), 1, 4, 4, 2, None) == capi.ERR_ARG
    assert L.cdll.clora_canny_emit(st.data_ptr(), None, None, 1, 4, 4, None) == capi.ERR_ARG


@pytest.mark.parametrize("case", IMAGES[:3] + IMAGES[5:], ids=lambda c: f"{c[1]}x{c[2]}x{c[3]}")
def test_composition_and_guide_tensor(case):
    img, lo, hi = _image(case)
    with use_emulator():
        cls = K.canny_classify(_batch(img), _thr(lo), _thr(hi))[0].numpy()
        edges = K.canny(torch.from_numpy(img), lo, hi)
        guide = K.canny(torch.from_numpy(img), lo, hi, guide=True)
    want = CC.hysteresis_np(cls)                                                         # numpy hysteresis of the DEVICE's class map
    assert edges.shape == img.shape[:2] and edges.dtype == torch.uint8 and np.array_equal(edges.numpy(), want)
    assert np.array_equal(want, P.canny(img, lo, hi))                                    # empty ambiguous mask: the shipped detector's map
    H, W = img.shape[:2]
    assert guide.shape == (1, 3, H, W) and guide.dtype == torch.float16
    assert set(guide.unique().tolist()) <= {-1.0, 1.0}
    assert torch.equal(guide[0, 0], guide[0, 1]) and torch.equal(guide[0, 0], guide[0, 2])
    assert torch.equal(guide[0, 0].float(), torch.from_numpy(want.astype(np.float32) / 127.5 - 1.0))


def test_wrappers_refuse_cpu_tensors_without_the_emulator():
    img, lo, hi = _image(IMAGES[1])
    if not torch.cuda.is_available():                 # product library + CPU tensors -> loud error, not a fallback
        with pytest.raises(capi.CloraError):
            K.canny(torch.from_numpy(img), lo, hi)
        with pytest.raises(capi.CloraError):
            K.canny_hysteresis(torch.ones(1, 4, 4, dtype=torch.uint8))


# ---------------------------------------------------------------- the data-set path
def _tok(caps):
    return torch.tensor([[len(c), sum(map(ord, c)) % 997] for c in caps])


def dataset_rows(n, w, h, seed=9, sigma=1.5):
    from PIL import Image
    rows = []
    for i in range(n):
        a = CC.noise_image(seed + i, h, w, 3, sigma)
        rows.append({"image": Image.fromarray(a, "RGB"), "prompt": f"prompt {i}"})
    return rows


def both_detectors(rows, resolution, device, seed=3):
    """the same seeded items through detector="numpy" and detector="device" -> (numpy batch, device batch, generator states)"""
    out, states = [], []
    for det in ("numpy", "device"):
        ds = P.DiffusionDBCanny(_tok, resolution=resolution, use_crop=True, rows=rows, detector=det)
        torch.manual_seed(seed)
        batch = data.collate([ds[i] for i in range(len(ds))])
        states.append(torch.get_rng_state())
        out.append(batch)
    assert "guide_values" in out[0] and "guide_values" not in out[1]
    assert out[1]["canny_image"].dtype == torch.uint8 and not out[1]["canny_image"].is_cuda
    return out[0], P.device_guides(out[1], device), states


def test_dataset_with_the_device_detector_gives_the_numpy_items():
    rows = dataset_rows(3, 100, 80)
    with use_emulator():
        ref, dev, states = both_detectors(rows, 64, "cpu")
    assert torch.equal(states[0], states[1])                                             # torch's generator consumed exactly alike
    assert set(dev) == set(ref) and "canny_image" not in dev
    assert torch.equal(dev["pixel_values"], ref["pixel_values"]) and torch.equal(dev["input_ids"], ref["input_ids"])
    assert dev["guide_values"].dtype == torch.float16 and dev["guide_values"].shape == ref["guide_values"].shape == (3, 3, 64, 64)
    assert torch.equal(dev["guide_values"].float(), ref["guide_values"])
    assert (ref["guide_values"] == 1).any()
    assert P.device_guides(ref, "cpu") is ref                                            # a batch without the fields is left alone
    with pytest.raises(ValueError):
        P.DiffusionDBCanny(_tok, rows=rows, detector="opencv")


def test_training_script_hands_the_detector_through_without_the_hub(monkeypatch):
    """`DiffusionDBCanny` without rows= would ask the hub for DiffusionDB: a subclass that supplies rows stands in under the same
    registry name (restored afterwards); parse_args takes the flag, build_dataset passes it on, and the script's batch-to-device
    step calls device_guides for such a batch and leaves every other batch alone"""
    import train_text_to_image_control_lora as T
    rows = dataset_rows(2, 80, 72)

    class Local(P.DiffusionDBCanny):
        def __init__(self, tokenizer, **kw):
            super().__init__(tokenizer, rows=rows, **kw)

    base = ["--pretrained_model_name_or_path", "x", "--control_lora_config", "c.json", "--resolution", "64"]
    a = T.parse_args(base + ["--dataset_name", "process/diffusiondb_canny"])
    assert a.canny_detector == "numpy"
    with pytest.raises(SystemExit):
        T.parse_args(base + ["--dataset_name", "process/diffusiondb_canny", "--canny_detector", "opencv"])
    monkeypatch.setitem(P.Dataset.DATASET_TYPE_DICT, "process/diffusiondb_canny", Local)
    assert T.build_dataset(a, _tok).detector == "numpy"
    a = T.parse_args(base + ["--dataset_name", "process/diffusiondb_canny", "--canny_detector", "device"])
    ds = T.build_dataset(a, _tok)
    assert isinstance(ds, Local) and ds.detector == "device" and ds.size == 64
    calls = []
    real = P.device_guides
    monkeypatch.setattr(P, "device_guides", lambda batch, dev: calls.append(dev) or real(batch, dev))
    torch.manual_seed(5)
    batch = data.collate([ds[0], ds[1]])
    with use_emulator():
        pixel, guide = T.batch_to_device(batch, "cpu")
    assert calls == ["cpu"] and pixel.dtype == guide.dtype == torch.float16 and guide.shape == (2, 3, 64, 64)
    torch.manual_seed(5)
    ref = data.collate([P.DiffusionDBCanny(_tok, resolution=64, rows=rows)[i] for i in range(2)])
    assert torch.equal(guide.float(), ref["guide_values"]) and torch.equal(pixel, ref["pixel_values"].half())
    pixel2, guide2 = T.batch_to_device(ref, "cpu")                                       # an ordinary batch: moved, nothing else
    assert calls == ["cpu"] and torch.equal(guide2, guide) and torch.equal(pixel2, pixel)
    # the other process/ data sets take no detector keyword
    a = T.parse_args(base + ["--dataset_name", "process/mpii_pose", "--canny_detector", "device"])
    seen = {}
    monkeypatch.setitem(P.Dataset.DATASET_TYPE_DICT, "process/mpii_pose", lambda tok, **kw: seen.update(kw) or "ds")
    assert T.build_dataset(a, _tok) == "ds" and "detector" not in seen


def test_app_detector_option():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("canny2image_dev", os.path.join(root, "apps", "canny2image.py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)
    img, lo, hi = _image(IMAGES[0])
    with use_emulator():
        got = app.detect(img, lo, hi, "device", device="cpu")
    assert np.array_equal(got, app.detect(img, lo, hi)) and np.array_equal(got, P.canny(img, lo, hi))
    with pytest.raises(ValueError):
        app.detect(img, lo, hi, "opencv")
