"""The host preparation of reef_ipa_check_batch (reef_amd/csrc/ipa_batch_host.inc) as a program of its own, no GPU: the build's
ipa_batch_selftest (REEF_BOUNDS: field.h checks its stated bounds as it goes), and the same source once more under the host sanitizers."""
import os
import subprocess

from reef_amd import _ffi

HOST_DIR = os.path.join(_ffi.CSRC, "host")


def test_the_selftest_of_the_build_passes():
    run = subprocess.run([os.path.join(os.path.dirname(_ffi.LIB_PATH), "ipa_batch_selftest")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "ipa_batch_selftest ok" in run.stdout, (run.stdout[-2000:], run.stderr[-2000:])


def test_the_preparation_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "ipa_batch_selftest_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DREEF_BOUNDS", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(HOST_DIR, "ipa_batch_selftest.cpp"), "-I" + os.path.dirname(_ffi.HEADER), "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stderr == "" and "ipa_batch_selftest ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
