"""CPU test: the host dispatch of clora_gemm_f16_ex, replayed against a recording.  tests/golden/gemm_dispatch_emu.json holds, for
every tile_cfg value 0..99 and every kind of launch whose path depends on the tile, the return code and the SHA-1 of every output
tensor on the emulator build (tools/gemm_dispatch_record.py, which also describes the kinds); the recording was made from the
library as it stood BEFORE the tile table replaced the hand-written switches and lists, so equality here is "the table dispatches
exactly as the lists did"."""
import importlib.util
import json
import os

from tests.emu_fixture import use_emulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_matches_the_recording(golden_dir):
    spec = importlib.util.spec_from_file_location("gemm_dispatch_record", os.path.join(ROOT, "tools", "gemm_dispatch_record.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    want = json.load(open(os.path.join(golden_dir, "gemm_dispatch_emu.json")))
    with use_emulator():
        got = rec.sweep()
    assert sorted(got) == sorted(want) and len(want) == 1500
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff
