"""CPU tier: the match tail of the K = 8 mismatch-line rows (csrc/fat_layout.h) -- table build, the
16-base trip of fat2_query.hip and the 16-element push of lane_out.h -- compiled against the SIMT
emulator with the trip counters in, compared with the oracle base by base with the tail on and off.
See tests/emu/match_tail_emu.py.  The library is built without sanitizers and nothing is preloaded."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def test_emulated_match_tail_matches_oracle_and_saves_trips():
    emu = os.path.join(HERE, "emu")
    subprocess.check_call(["make", "-C", emu, "-f", "match_tail_emu.mk", "libcolbwt_emu_trips.so"], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    for k in ("COLBWT_MATCH_TAIL", "COLBWT_LINE_ROWS_CHUNK", "COLBWT_LAYOUT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(emu, "match_tail_emu.py")], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "MATCH-TAIL-EMU-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
