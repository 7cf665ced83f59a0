"""The lookup leg of the replay (`reef_replay cfgN lookup`, reef_amd/csrc/host/replay_lookup.hpp) on the host: its exports, and its
checks (host/lookup_check.hpp) run on a tiny honest transcript made on the host with plain loops -- every round's sum-check equations,
the challenges, T~ at the step's point, the running claim from step to step, the claim handed to the consistency argument and the Hyrax
argument -- which they must accept and, with one recorded value altered, reject naming the phase.  The transcript the self-test prints
is recomputed here with the reference restatement oracle/sumcheck_oracle.py.  No GPU: libreef_replay.so loads without one."""
import ctypes
import inspect
import json
import os
import subprocess

import pytest

from oracle import sumcheck_oracle as S
from reef_amd import _ffi, replay

Q = S.Q
EXE = os.path.join(os.path.dirname(replay.LIB_PATH), "lookup_check_selftest")
HOST_DIR = os.path.join(_ffi.CSRC, "host")


def _ints(xs):
    return [int(x, 16) for x in xs]


def test_the_lookup_exports_and_the_python_front_end_exist():
    lib = ctypes.CDLL(replay.LIB_PATH)
    for name in ("reef_replay_run_lookup", "reef_replay_lookup_selftest", "reef_replay_run_prove", "reef_replay_check_selftest"):
        assert hasattr(lib, name), name
    assert replay.LOOKUP_PHASES == ("lookup", "claim", "hyrax")
    sig = inspect.signature(replay.run_lookup)
    assert list(sig.parameters) == ["config", "mode", "proj", "width", "tamper", "shapes_path"]
    assert [p.default for p in sig.parameters.values()] == ["cfg3", None, 0, 1, None, None]
    assert list(inspect.signature(replay.lookup_selftest).parameters) == ["tamper"]
    # the prove leg's front end is as it was
    assert list(inspect.signature(replay.run_prove).parameters) == ["config", "tamper", "tables", "shapes_path"]
    assert replay.PROVE_PHASES == ("nifs", "spartan", "open", "hyrax")
    with pytest.raises(ValueError):
        replay.run_lookup("cfg1", tamper="everything")


def test_both_forms_accept_the_honest_transcript():
    out = replay.lookup_selftest()
    assert out["selftest"] == "accepted" and out["tamper"] == ""
    assert (out["ell"], out["steps"], out["lookups"]) == (4, 3, 3)
    assert out["rounds_checked"] == 2 * 3 * 4 and out["values_checked"] == 2 * 3 * 3      # two modes
    run = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and json.loads(run.stdout) == out


@pytest.mark.parametrize("phase", ["lookup", "claim", "hyrax"])
def test_the_checks_reject_a_tampered_transcript_naming_the_phase(phase):
    with pytest.raises(replay.ProofRejected) as e:
        replay.lookup_selftest(phase)
    assert e.value.phase == phase and str(e.value).startswith(f"proof check failed [{phase}]")
    run = subprocess.run([EXE, phase], capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and run.stdout.startswith(f"proof check failed [{phase}]"), run.stdout


def test_the_host_only_checker_program_agrees_with_the_library():
    """lookup_check_selftest is lookup_check.hpp linked WITHOUT libreef_msm.so (host/Makefile): the same exit code and the same line
    as the library's entry point, for an honest transcript, every tampered phase and an unknown one (a usage error: 2)."""
    for arg, rc in [("", 0), ("lookup", 1), ("claim", 1), ("hyrax", 1), ("bogus", 2)]:
        run = subprocess.run([EXE] + ([arg] if arg else []), capture_output=True, text=True, timeout=60)
        buf = ctypes.create_string_buffer(65536)
        assert replay._load().reef_replay_lookup_selftest(arg.encode(), buf, len(buf)) == rc, arg
        assert run.returncode == rc, (arg, run.stderr)
        assert run.stdout == buf.value.decode() + "\n", arg
    assert "one of lookup, claim, hyrax" in run.stdout


@pytest.mark.parametrize("mode", ["doc", "hybrid"])
def test_the_printed_transcript_is_the_reference_restatements(mode):
    """Every (xsq, x, con), every next_running_v and the hybrid identity of the line recomputed with gen_eq_table, linear_mle_coeffs,
    linear_mle_fold and verifier_mle_eval; the challenges are taken from the line (the stand-in transcript is not restated here)."""
    line = replay.lookup_selftest()
    ell, rec = line["ell"], line["modes"][mode]
    table = _ints(rec["table"])
    assert len(table) == 1 << ell
    prev_q, prev_v = [0] * ell, table[0]
    for st in rec["steps"]:
        qs, vs = st["qs"], _ints(st["vs"])
        assert vs == [table[q] for q in qs]
        assert _ints(st["prev_q"]) == prev_q and int(st["prev_v"], 16) == prev_v
        claim_r = int(st["claim_r"], 16)
        rs = [pow(claim_r, i + 1, Q) for i in range(len(qs) + 1)]
        t = list(table)
        e = S.gen_eq_table(rs, qs, list(reversed(prev_q)), Q)                                # r1cs.rs:2319
        sc_rs = _ints(st["sc_rs"])
        claim = (sum(r * v for r, v in zip(rs, vs)) + rs[-1] * prev_v) % Q
        for i in range(1, ell + 1):
            xsq, x, con = S.linear_mle_coeffs(t, e, ell, i, Q)
            assert _ints(st["g"][i - 1]) == [xsq, x, con], (mode, i)
            assert (2 * con + x + xsq) % Q == claim
            r = sc_rs[i - 1]
            claim = (xsq * r * r + x * r + con) % Q
            S.linear_mle_fold(t, e, ell, i, r, Q)
        next_v = int(st["next_v"], 16)
        assert next_v == t[0] == S.verifier_mle_eval(table, sc_rs, Q)                        # r1cs.rs:2379-2385
        assert claim == next_v * e[0] % Q
        prev_q, prev_v = sc_rs, next_v
    ev = int(rec["eval"], 16)
    if mode == "doc":
        assert ev == prev_v
    else:
        half = 1 << (ell - 1)
        q0, t_pub = int(rec["q0"], 16), int(rec["t"], 16)
        assert q0 == prev_q[0]
        assert t_pub == S.verifier_mle_eval(table[:half], prev_q[1:], Q)                      # commitment.rs:237-238
        assert ev == S.verifier_mle_eval(table[half:], prev_q[1:], Q)                         # doc_poly.evaluate(running_q)
        assert ((1 - q0) * t_pub + q0 * ev) % Q == prev_v                                     # commitment.rs:241-244
        assert len(set(table[rec["public"]:half])) == 1                                       # one fill value up to the half


def test_the_checker_under_host_sanitizers(tmp_path):
    """lookup_check_selftest once more with -fsanitize=address,undefined, as a program of its own: clean with no argument and with
    every tamper (a rejection still exits 1; a sanitizer report would exit otherwise or write to stderr)."""
    exe = str(tmp_path / "lookup_check_selftest_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(HOST_DIR, "lookup_check_selftest.cpp"), "-I" + os.path.dirname(_ffi.HEADER), "-o", exe], check=True, timeout=300)
    for arg, rc in [("", 0), ("lookup", 1), ("claim", 1), ("hyrax", 1)]:
        run = subprocess.run([exe] + ([arg] if arg else []), capture_output=True, text=True, timeout=120)
        assert run.returncode == rc and run.stderr == "", (arg, run.returncode, run.stderr[-2000:])
