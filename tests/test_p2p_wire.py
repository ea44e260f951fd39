"""The one-sided transfer's wire records (csrc/p2p_wire.h) parse bytes that came from another process.
tests/p2p_wire_check.cpp exercises them on the CPU -- round trips, every strict prefix of a valid pull
record, each poisoned count -- built with AddressSanitizer and UBSan and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_p2p_wire_under_sanitizers(tmp_path):
    exe = str(tmp_path / "p2p_wire_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tests", "p2p_wire_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "p2p_wire: ok" in run.stdout
