"""CPU suite: `--verify-scripts` of the command-line compressor is announced with exactly what it covers, and parsed before a GPU is touched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "colord_amd", "colord_hip")
COVERS = "every read is rebuilt on the device from its edit script and the reference reads and compared with the input; the entropy-coded bytes are not decoded"


def test_usage_lists_verify_scripts_and_what_it_covers():
    r = subprocess.run([CLI], capture_output=True, text=True)
    assert "--verify-scripts" in r.stderr
    assert COVERS in " ".join(r.stderr.split())
    assert "--verify " not in r.stderr


def test_verify_scripts_is_an_option_of_the_compress_modes():
    # accepted as an option: the complaint is about the paths, not about the option
    r = subprocess.run([CLI, "compress-ont", "--verify-scripts", "in.fq"], capture_output=True, text=True)
    assert r.returncode == 1 and "expected input and output paths" in r.stderr and "unknown option" not in r.stderr


def test_binding_declares_the_new_entry_points():
    from colord_amd import _native as N
    lib = N.load()
    for name in ("cl_es_expand", "cl_es_verify", "cl_ctx_set_verify", "cl_ctx_verified", "cl_compressor_verified"):
        assert name in N.exported_names() and hasattr(lib, name)
    assert N.CL_E_MISMATCH == -6
