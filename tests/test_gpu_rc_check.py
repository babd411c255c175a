"""The coded-part check's kernel alone (k_range_check, csrc/rc_check.hpp) against the oracle's DECODER (oracle/rc.h: orc_rcd_start / _cum /
_update, the restatement of sub_rc.h:216-392): 150 parts in three groups (one of parts with whole rounds, one of empty parts, a ragged one
with the round edges 0, 1, 2, 7, 8, 9, 23, 24, 25, 47, 48, 49), totals over the whole 21-bit range and at the extremes, coded by
k_range_code, packed back to back at unaligned offsets beyond 2^31 — clean, with a flipped bit, with sizes one off, with a shifted or empty
interval, with sizes of ~0 and a buffer that ends inside a part: first_bad equals the oracle's answer element for element and nothing is
written outside it.  The same cases run on the CPU through the shared step (test_verify_streams_cpu.py)."""
import os
import shutil
import subprocess
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_range_check_kernel_equals_the_oracle_decoder(tmp_path):
    exe = str(tmp_path / "rc_check_test")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tools", "rc_check_test.hip"), "-o", exe])
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ok:" in r.stdout, "exit %d\n" % r.returncode + r.stdout[-2000:] + r.stderr[-2000:]
