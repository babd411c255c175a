"""CPU suite for the opt-in check of the coded parts (`colord_hip compress-* --verify-streams` / cl_ctx_set_verify_streams): the option is
announced with exactly what it covers and what it does not, parsed before a GPU is touched, bound in Python — and the per-symbol step
that the kernel k_range_check and host loops share (rc_check_step, csrc/rc_check.hpp) equals the oracle's decoder on the cases of the
GPU program, under AddressSanitizer and UBSan, as a stand-alone program."""
import os
import shutil
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
COVERS = ("each coded part of the dna and qual streams is decoded on the device with the decoder's interval arithmetic: every symbol must fall in the interval "
          "its model gave it and the part must end at its size")
NOT_COVERED = "the models themselves are not replayed"
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
# the sanitizers' runtimes linked INTO the program (gcc links them dynamically unless told; clang statically anyway)
STATIC_RT = ["-static-libasan", "-static-libubsan"] if CXX and "clang" not in os.path.basename(CXX) else []


def test_usage_lists_verify_streams_and_what_it_covers():
    r = subprocess.run([CLI], capture_output=True, text=True)
    usage = " ".join(r.stderr.split())
    assert "--verify-streams" in r.stderr
    assert COVERS in usage
    assert NOT_COVERED in usage
    assert "--verify " not in r.stderr


def test_verify_streams_is_an_option_of_the_compress_modes():
    # accepted as an option: the complaint is about the paths, not about the option
    r = subprocess.run([CLI, "compress-ont", "--verify-streams", "in.fq"], capture_output=True, text=True)
    assert r.returncode == 1 and "expected input and output paths" in r.stderr and "unknown option" not in r.stderr


def test_binding_declares_the_new_entry_points():
    from colord_amd import _native as N
    lib = N.load()
    for name in ("cl_ctx_set_verify_streams", "cl_ctx_verified_streams", "cl_compressor_verified_streams"):
        assert name in N.exported_names() and hasattr(lib, name)
    from colord_amd import device as D
    assert hasattr(D.Context, "set_verify_streams") and hasattr(D.Context, "verified_streams") and hasattr(D.Compressor, "verified_streams")


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_shared_step_equals_the_oracle_decoder_on_the_host_under_sanitizers(tmp_path):
    # the header compiles for the host without HIP (RC_CHECK_HOST_ONLY); the program has its own main and runs as it is, nothing preloaded
    exe = str(tmp_path / "rc_check_host_test")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + STATIC_RT + [
                           os.path.join(ROOT, "tests", "tools", "rc_check_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok:" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
