"""Record what the reference computes on the small cases of tests/test_oracle.py and tests/test_process_datasets_cpu.py
(reference models.py / process/*.py imported in place, nothing copied) -> tests/golden/reference_records.{safetensors,json}.
The tests compare the restatement and this repository's classes with that record, so they need no reference checkout.

    python -m oracle.make_reference_records REFERENCE_ROOT          (a checkout of the reference repository)
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cases, unet_ref  # noqa: E402
from oracle.diffusers_shim import import_reference_models  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_records")
CONFIGS = ["fill50k", "diffusiondb-canny", "mpii-pose", "post-add", "danbooru-sketch", "mpii-pose-v2", "diffusiondb-canny-v2"]


def record_adapter_chain(ref, out):
    """the procedure of the former in-place test: seeded weights, a pre and a post LoRA chained to each control processor"""
    from tests.test_oracle import chain_modules
    for case in ("v1", "v2"):
        torch.manual_seed(0)
        unet_ref.CrossAttention(64, None, heads=4, dim_head=16)              # drawn first, as the in-place test did
        for self_attn in (True, False):
            head = f"chain.{case}.{'self' if self_attn else 'cross'}."
            cad = None if self_attn else 48
            attn = unet_ref.CrossAttention(64, cad, heads=4, dim_head=16)
            a, pre_a, post_a = chain_modules(ref, case, cad)
            for m, s in ((a, 1), (pre_a, 2), (post_a, 3)):
                cases.seeded_weights_(m, seed=s)
            for name, m in (("attn", attn), ("proc", a), ("pre", pre_a), ("post", post_a)):
                for k, v in m.state_dict().items():
                    out[head + name + "." + k] = v.detach().clone().contiguous()
            a.inject_pre_lora(pre_a); a.inject_post_lora(post_a)
            h = torch.randn(2, 16, 64)
            e = None if self_attn else torch.randn(2, 5, 48)
            ctrl = torch.randn(1, 64 if case == "v1" else 32, 4, 4)       # control batch 1 broadcasts (C6)
            a.inject_control_states(ctrl)
            with torch.no_grad():
                y = a(attn, h, e, None, 0.7)
            out[head + "h"], out[head + "ctrl"], out[head + "y"] = h, ctrl.clone(), y.detach().contiguous()
            if e is not None:
                out[head + "e"] = e


def record_configs(ref, reference_root, meta):
    for name in CONFIGS:
        path = os.path.join(reference_root, "configs", f"{name}.json")
        with open(path) as f:
            cfg = json.load(f)
        m = ref.ControlLoRA.from_config(path)
        meta[f"configs.{name}"] = {"config": cfg, "n_params": sum(p.numel() for p in m.parameters()),
                                   "state_dict_shapes": {k: list(v.shape) for k, v in m.state_dict().items()}}


def record_process(reference_root, out, meta):
    from tests import test_process_datasets_cpu as T
    with pytest.MonkeyPatch.context() as mp, tempfile.TemporaryDirectory() as tmp:
        T.make_tree(Path(tmp))
        mp.chdir(tmp)
        proc = T.import_reference_process(mp, reference_root)
        ds = proc("mpii_pose").Dataset(T._tok, resolution=64, use_crop=True)
        meta["process.mpii_pose.len"] = len(ds)
        T.record_items(meta, "process.mpii_pose.crop", ds, 3, 11)
        T.record_items(meta, "process.mpii_pose.nocrop", proc("mpii_pose").Dataset(T._tok, resolution=64, use_crop=False), 3, 2)
        ds = proc("danbooru_sketch").Dataset(T._tok, resolution=64, use_crop=True)
        meta["process.danbooru_sketch.sketch_styles"] = list(ds.sketch_styles)
        T.record_items(meta, "process.danbooru_sketch", ds, 2, 7)
        rows = T.canny_rows()
        import datasets.load
        mp.setattr(datasets.load, "load_dataset", lambda *a, **k: {"train": rows})
        proc = T.import_reference_process(mp, reference_root)      # fresh import: the module binds load_dataset when it loads
        T.record_items(meta, "process.diffusiondb_canny", proc("diffusiondb_canny").Dataset(T._tok, resolution=64, use_crop=True), 3, 3)
        img, tgt, gd = T.cat_input_case()
        out["process.cat_input"] = torch.from_numpy(np.asarray(proc("base").Dataset.cat_input(img, tgt, gd)).copy())


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: python -m oracle.make_reference_records REFERENCE_ROOT (a checkout of the reference repository)")
    reference_root = sys.argv[1]
    ref = import_reference_models(reference_root)
    out, meta = {}, {}
    record_adapter_chain(ref, out)
    record_configs(ref, reference_root, meta)
    record_process(reference_root, out, meta)
    save_file(out, OUT + ".safetensors")
    with open(OUT + ".json", "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} tensors, {len(meta)} entries -> {OUT}.{{safetensors,json}}")


if __name__ == "__main__":
    main()
