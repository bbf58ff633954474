"""CPU tier: the persistent-lane query kernels' multi-read chunks (csrc/fat_cursor.h ChunkPlan /
ReadCursor and the wave collectors) on ragged batches, compiled against the SIMT emulator with
ASan/UBSan and compared with the oracle base by base.  See tests/emu/chunk_emu.py."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def test_emulated_multi_read_chunks_on_ragged_batches():
    emu = os.path.join(HERE, "emu")
    subprocess.check_call(["make", "-C", emu, "libcolbwt_emu.so"], stdout=subprocess.DEVNULL)
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"]).decode().strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0")
    env.pop("COLBWT_LINE_ROWS_CHUNK", None)
    out = subprocess.run([sys.executable, os.path.join(emu, "chunk_emu.py")], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "CHUNK-EMU-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
