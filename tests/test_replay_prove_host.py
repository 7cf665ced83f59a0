"""The prove leg of the replay (reef_amd/csrc/host/reef_replay.cpp, `reef_replay cfgN prove`) on the host: its exports, and its
checks (host/proof_check.hpp) run on a tiny honest transcript made on the host -- the NIFS bookkeeping, the two sum-check identities, the verifier's sparse
evaluation and the IPA identities of the opening and of the Hyrax argument -- which they must accept, and, with one recorded value
altered, reject naming the phase.  No GPU: libreef_replay.so loads without one."""
import ctypes
import inspect
import os
import subprocess

import pytest

from reef_amd import replay


def test_the_prove_exports_exist():
    lib = ctypes.CDLL(replay.LIB_PATH)
    for name in ("reef_replay_run_prove", "reef_replay_check_selftest", "reef_replay_run", "reef_replay_run_devices"):
        assert hasattr(lib, name), name


def test_the_checks_accept_an_honest_transcript():
    out = replay.check_selftest()
    assert out["selftest"] == "accepted" and out["tamper"] == ""
    # 16 = the padded sizes of the tiny shape: log2 16 outer rounds, log2 (2 * 16) inner ones, log2 16 IPA rounds; 2^6 = 8 x 8 document
    assert (out["outer_rounds"], out["inner_rounds"], out["ipa_rounds"], out["hyrax_rounds"]) == (4, 5, 4, 3)
    assert out["nnz"] > 3 * out["num_cons"] // 2


@pytest.mark.parametrize("phase", ["nifs", "spartan", "open", "hyrax"])
def test_the_checks_reject_a_tampered_transcript_naming_the_phase(phase):
    with pytest.raises(replay.ProofRejected) as e:
        replay.check_selftest(phase)
    assert e.value.phase == phase and f"[{phase}]" in str(e.value)


def test_an_unknown_tamper_phase_is_a_usage_error():
    with pytest.raises(ValueError):
        replay.run_prove("cfg1", tamper="everything")
    buf = ctypes.create_string_buffer(512)
    assert replay._load().reef_replay_check_selftest(b"everything", buf, len(buf)) == 2
    assert b"one of nifs, spartan, open, hyrax" in buf.value


def test_the_host_only_checker_program_agrees_with_the_library():
    """proof_check_selftest is proof_check.hpp linked WITHOUT libreef_msm.so (host/Makefile): the same exit code and the same line as
    the library's entry point, for an honest transcript, every tampered phase and a usage error."""
    exe = os.path.join(os.path.dirname(replay.LIB_PATH), "proof_check_selftest")
    for arg, rc in [("", 0), ("nifs", 1), ("spartan", 1), ("open", 1), ("hyrax", 1), ("bogus", 2)]:
        run = subprocess.run([exe, arg], capture_output=True, text=True, timeout=60)
        buf = ctypes.create_string_buffer(4096)
        assert replay._load().reef_replay_check_selftest(arg.encode(), buf, len(buf)) == rc, arg
        assert run.returncode == rc, (arg, run.stderr)
        assert run.stdout == buf.value.decode() + "\n", arg


def test_the_call_order_of_the_resident_proof_contexts():
    """proof_order_selftest is csrc/proof_order.h alone (host/Makefile: no HIP, no library): every phase of the Spartan sum-checks with
    the opening and of the Hyrax argument against every call of the family, with a table written out in the program -- accept or
    refuse, the full error text and the phase reset.  One line, exit 1 on a mismatch."""
    exe = os.path.join(os.path.dirname(replay.LIB_PATH), "proof_order_selftest")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("proof_order_selftest: ok, ") and run.stdout.count("\n") == 1, run.stdout


def test_the_msm_replay_defaults_are_unchanged():
    """bench.py calls replay.run(cfg, nofold=True, tables=...): the prove leg is a separate entry point, opt-in."""
    sig = inspect.signature(replay.run)
    assert list(sig.parameters) == ["config", "nofold", "tables", "shapes_path", "devices"]
    assert [sig.parameters[k].default for k in sig.parameters] == ["cfg3", True, False, None, None]
    assert list(inspect.signature(replay.run_prove).parameters) == ["config", "tamper", "tables", "shapes_path"]
