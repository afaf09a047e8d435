"""Record what the reference computes when a chained member is itself a control processor (reference models.py:232-243 for v1,
:366-372 and :412-418 for V2) -> tests/golden/multi_control_records.safetensors.  The reference's models.py is imported in place
through oracle.diffusers_shim, nothing is copied.  tests/multi_control_cases.py reads the file (load_records) and builds the same
chains from the oracle's and from this repository's classes, so the tests need no reference checkout.

    python tools/make_multi_control_records.py REFERENCE_ROOT          (a checkout of the reference repository)

Geometry of oracle/make_reference_records.record_adapter_chain: C 64, 4 heads, ctx 48, 16 tokens, UNet batch 2, scale 0.7, seeded
weights.  Weights and inputs are fp16 values (stored as fp16), so the product's fp16 operands hold exactly what the reference
computed with; the recorded outputs are fp32.  What records share is stored once: the two attention modules, h, e, and a case's
processor weights for its two control batches."""
from __future__ import annotations

import os
import sys

import torch
from safetensors.torch import save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cases, unet_ref  # noqa: E402
from oracle.diffusers_shim import import_reference_models  # noqa: E402
from tests import multi_control_cases as MC  # noqa: E402

UP_STD = 0.2


def _seed_fp16(module, seed):
    cases.seeded_weights_(module, seed=seed, up_std=UP_STD)
    with torch.no_grad():
        for q in module.parameters():
            q.copy_(q.half().float())


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: python tools/make_multi_control_records.py REFERENCE_ROOT (a checkout of the reference repository)")
    ref = import_reference_models(sys.argv[1])
    mods = dict(control=ref.ControlLoRACrossAttnProcessor, control_v2=ref.ControlLoRACrossAttnProcessorV2,
                plain=ref.LoRACrossAttnProcessor)
    G = MC.GEOM
    C, B, N, ctx, side = G["C"], G["B"], G["N"], G["ctx"], 4
    g = torch.Generator().manual_seed(0)
    out = {"shared/h": torch.randn(B, N, C, generator=g).half(), "shared/e": torch.randn(B, 5, ctx, generator=g).half()}
    attns = {}
    for where, cad in (("self", None), ("cross", ctx)):
        attn = unet_ref.CrossAttention(C, cad, heads=G["heads"], dim_head=C // G["heads"])
        _seed_fp16(attn, seed=5)
        attns[where] = attn
        for k, v in attn.state_dict().items():
            out[f"attn.{where}/{k}"] = v.detach().half().contiguous()
    for case in MC.RECORD_CASES:
        cc = C if case.startswith("v1") else G["ctrl_c_v2"]
        for where, cad in (("self", None), ("cross", ctx)):
            main_p, members = MC.record_chain(case, where == "self", mods)
            for i, m in enumerate([main_p] + members):
                _seed_fp16(m, seed=1 + i)
                name = "main" if i == 0 else f"member{i - 1}"
                for k, v in m.state_dict().items():
                    out[f"w.{case}:{where}/{name}.{k}"] = v.detach().half().contiguous()
            for cb in (1, B):
                head = f"{case}:{where}:cb{cb}/"
                ctrl = torch.randn(cb, cc, side, side, generator=g).half()
                out[head + "ctrl.main"] = ctrl
                main_p.inject_control_states(ctrl.float())
                for i, m in enumerate(members):
                    if hasattr(m, "inject_control_states"):
                        c = torch.randn(cb, cc, side, side, generator=g).half()
                        out[head + f"ctrl.member{i}"] = c
                        m.inject_control_states(c.float())
                with torch.no_grad():
                    y = main_p(attns[where], out["shared/h"].float(), out["shared/e"].float() if cad else None, None, G["scale"])
                out[head + "y"] = y.detach().float().contiguous()
    save_file(out, MC.RECORDS)
    size = os.path.getsize(MC.RECORDS)
    print(f"{len(out)} tensors, {size} bytes -> {MC.RECORDS}")
    assert size < 1_000_000, "the fixture must stay below 1 MB"


if __name__ == "__main__":
    main()
