"""The `process/<name>` data sets (controllora_amd/process.py) against the reference's own classes executed in place
(reference process/base.py:8-38, diffusiondb_canny.py:11-48, mpii_pose.py:10-46, danbooru_sketch.py:9-76).

The reference modules need `jsonlines`, `cv2` and a reachable DiffusionDB; the test provides a six-line `jsonlines` stand-in, routes
`cv2.Canny` to this repo's numpy Canny (so what is compared for that class is everything AROUND the detector: crop, draw order of
the random thresholds, scaling, channel replication) and hands `load_dataset` a local list.  The reference's items on these inputs are
recorded in tests/golden/reference_records.safetensors (`python -m oracle.make_reference_records`, which runs the reference's classes in
place with the same stand-ins); the tests compare this repository's classes with that record."""
import hashlib
import importlib
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

from safetensors.torch import load_file

from controllora_amd import process as P

RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_records")


def _tok(x):
    """both calling conventions: examples dict (reference) / caption list (this repo)"""
    caps = x["text"] if isinstance(x, dict) else x
    return torch.tensor([[len(c), sum(map(ord, c)) % 997] for c in caps])


def _rand_img(rng, w, h, mode="RGB"):
    a = rng.integers(0, 256, size=(h, w, 3) if mode == "RGB" else (h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    blob = ((xx - w / 2) ** 2 + (yy - h / 2) ** 2 < (min(w, h) / 3) ** 2)
    a = np.where(blob[..., None] if mode == "RGB" else blob, a // 4, 128 + a // 2).astype(np.uint8)     # structure for the edge detector
    return Image.fromarray(a, mode)


@pytest.fixture()
def tree(tmp_path, monkeypatch):
    make_tree(tmp_path)
    monkeypatch.chdir(tmp_path)
    return tmp_path


def make_tree(tmp_path):
    """data/mpii + data/danbooru-2020-512{,-style} under `tmp_path` (a pathlib.Path), as the reference expects them"""
    rng = np.random.default_rng(5)
    (tmp_path / "data" / "mpii" / "img").mkdir(parents=True)
    recs = []
    for i, (w, h) in enumerate([(96, 80), (64, 64), (70, 100)]):
        _rand_img(rng, w, h).save(tmp_path / "data" / "mpii" / "img" / f"{i}.png")
        _rand_img(rng, w, h).save(tmp_path / "data" / "mpii" / "img" / f"{i}_pose.png")
        recs.append({"image": f"img/{i}.png", "guide": f"img/{i}_pose.png", "text": f"a person number {i}"})
    (tmp_path / "data" / "mpii" / "prompt.jsonl").write_text("\n".join(json.dumps(r) for r in recs) + "\n")
    recs = []
    for style in ("", "-illyasviel", "-erika", "-infor"):
        (tmp_path / "data" / f"danbooru-2020-512{style}" / "0").mkdir(parents=True)
    for i, (w, h) in enumerate([(90, 72), (64, 64)]):
        _rand_img(rng, w, h).save(tmp_path / "data" / "danbooru-2020-512" / "0" / f"{i}.png")
        for style in ("illyasviel", "erika", "infor"):
            _rand_img(rng, w, h, "L").save(tmp_path / "data" / f"danbooru-2020-512-{style}" / "0" / f"{i}.png")
        recs.append({"image": f"danbooru-2020-512/0/{i}.png", "text": f"1girl, sketch {i}"})
    (tmp_path / "data" / "danbooru-2020-512-prompt.jsonl").write_text("\n".join(json.dumps(r) for r in recs) + "\n")


def import_reference_process(monkeypatch, reference_root):
    """import the reference's `process` package where it lies, with stand-ins for the three things this image lacks (used by
    oracle/make_reference_records.py to record the reference's items)"""

    class _Reader:
        def __init__(self, f):
            self._rows = [json.loads(l) for l in f if l.strip()]
        def __iter__(self):
            return iter(self._rows)
        def __enter__(self):
            return self
        def __exit__(self, *a):
            return False
    jl = types.ModuleType("jsonlines")
    jl.Reader = _Reader
    jl.open = lambda path, mode="r": _Reader(open(path, "r"))
    cv2 = types.ModuleType("cv2")
    cv2.Canny = lambda img, lo, hi: P.canny(img, min(lo, hi), max(lo, hi))
    monkeypatch.setitem(sys.modules, "jsonlines", jl)
    monkeypatch.setitem(sys.modules, "cv2", cv2)
    monkeypatch.syspath_prepend(reference_root)
    for m in [k for k in sys.modules if k == "process" or k.startswith("process.")]:
        monkeypatch.delitem(sys.modules, m)
    return lambda name: importlib.import_module("process." + name)


def draw_items(ds, n, seed):
    """items 0..n-1 and item 0 once more after torch.manual_seed(seed), and the torch RNG state after them"""
    torch.manual_seed(seed)
    items = [ds[i] for i in range(n)] + [ds[0]]
    return items, torch.get_rng_state()


def digest(t):
    """dtype, shape and SHA-256 of the values (-0.0 counted as 0.0, as torch.equal does): an exact comparison that keeps the
    recorded items small"""
    t = t.detach().contiguous()
    if t.is_floating_point():
        t = t + 0.0
    return {"dtype": str(t.dtype), "shape": list(t.shape), "sha256": hashlib.sha256(t.numpy().tobytes()).hexdigest(),
            "sum": float(t.double().sum())}


def record_items(meta, prefix, ds, n, seed):
    """what draw_items gives for the reference's class, as digests in `meta` under `prefix`"""
    items, state = draw_items(ds, n, seed)
    meta[prefix] = {"items": [{k: digest(v) for k, v in x.items()} for x in items], "rng_state": digest(state)}


def _records():
    with open(RECORDS + ".json") as f:
        meta = json.load(f)
    return load_file(RECORDS + ".safetensors"), meta


def _same_items(mine, prefix, n, seed):
    rec = _records()[1][prefix]
    a, state_a = draw_items(mine, n, seed)
    assert digest(state_a) == rec["rng_state"], "a different number of random draws than the reference"
    assert len(a) == len(rec["items"]) == n + 1
    for x, y in zip(a, rec["items"]):
        assert set(x) == set(y) == {"pixel_values", "guide_values", "input_ids"}
        for k in x:
            d = digest(x[k])
            assert d["dtype"] == y[k]["dtype"] and d["shape"] == y[k]["shape"], k
            assert d == y[k], (k, d["sum"], y[k]["sum"])


def test_registry_names_and_lookup():
    assert set(P.Dataset.DATASET_TYPE_DICT) == {"process/diffusiondb_canny", "process/mpii_pose", "process/danbooru_sketch"}
    assert P.Dataset.from_name("process/mpii_pose") is P.MPIIPose
    assert P.MPIIPose.control_channel() == 3
    with pytest.raises(KeyError, match="registered"):
        P.Dataset.from_name("process/nope")


def test_mpii_pose_items_equal_the_reference_class(tree):
    mine = P.Dataset.from_name("process/mpii_pose")(_tok, resolution=64, use_crop=True)
    assert len(mine) == _records()[1]["process.mpii_pose.len"] == 3
    _same_items(mine, "process.mpii_pose.crop", 3, seed=11)
    _same_items(P.MPIIPose(_tok, resolution=64, use_crop=False), "process.mpii_pose.nocrop", 3, seed=2)


def test_danbooru_sketch_items_equal_the_reference_class(tree):
    mine = P.DanbooruSketch(_tok, resolution=64, use_crop=True)
    assert mine.SKETCH_STYLES == tuple(_records()[1]["process.danbooru_sketch.sketch_styles"])
    _same_items(mine, "process.danbooru_sketch", 2, seed=7)


def canny_rows():
    rng = np.random.default_rng(9)
    return [{"image": _rand_img(rng, w, h), "prompt": f"prompt {i}"} for i, (w, h) in enumerate([(100, 80), (64, 64), (64, 90)])]


def test_diffusiondb_canny_pipeline_equals_the_reference_class_around_the_detector():
    mine = P.DiffusionDBCanny(_tok, resolution=64, use_crop=True, rows=canny_rows())
    _same_items(mine, "process.diffusiondb_canny", 3, seed=3)


def test_canny_item_is_a_three_channel_edge_map_with_seeded_thresholds():
    rng = np.random.default_rng(1)
    rows = [{"image": _rand_img(rng, 80, 72), "prompt": "x"}]
    ds = P.DiffusionDBCanny(_tok, resolution=64, rows=rows)
    torch.manual_seed(0)
    a = ds[0]
    torch.manual_seed(0)
    b = ds[0]
    assert torch.equal(a["guide_values"], b["guide_values"]) and a["guide_values"].shape == (3, 64, 64)
    g = a["guide_values"]
    assert set(g.unique().tolist()) <= {-1.0, 1.0} and torch.equal(g[0], g[1]) and torch.equal(g[0], g[2])
    assert a["pixel_values"].min() >= -1 and a["pixel_values"].max() <= 1


def cat_input_case():
    img = _rand_img(np.random.default_rng(2), 48, 40)
    g = torch.Generator().manual_seed(4)
    return img, torch.rand(1, 3, 20, 24, generator=g) * 2 - 1, torch.rand(1, 3, 20, 24, generator=g) * 2 - 1


def test_cat_input_strip_matches_the_reference_layout():
    img, tgt, gd = cat_input_case()
    mine = P.Dataset.cat_input(img, tgt, gd)
    assert mine.size == (144, 40)
    ref = _records()[0]["process.cat_input"]
    assert np.array_equal(np.asarray(mine), ref.numpy())


def test_train_script_selects_process_datasets(tree):
    import train_text_to_image_control_lora as T
    args = types.SimpleNamespace(dataset_name="process/mpii_pose", resolution=64, max_train_samples=None, seed=0)
    ds = T.build_dataset(args, _tok)
    assert isinstance(ds, P.MPIIPose) and len(ds) == 3
    from controllora_amd import data
    batch = data.collate([ds[1], ds[1]])
    assert batch["pixel_values"].shape == (2, 3, 64, 64) and batch["input_ids"].shape == (2, 2)
