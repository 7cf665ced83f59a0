"""ctypes front-end of libreef_replay.so: the MSM sequence of one `reef --prove` run (eniac/Reef
src/backend/framework.rs:642-754) issued through the C ABI by the C++ harness reef_amd/csrc/host/reef_replay.cpp.

The harness is host code of the product side (it links libreef_msm.so only); its MSM lengths come from
tests/golden/replay_shapes.json, which oracle/gen_replay_shapes.py derives from Reef's cost model.  Every per-step
commitment is checked inside the harness against its discrete-logarithm closed form; a mismatch is an error here.
run_prove() is the harness's prove leg: every device row of one proof on synthetic R1CS, checked with the verifier's equations.
"""
from __future__ import annotations

import ctypes
import functools
import json
import os

from . import _ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libreef_replay.so")
SHAPES_PATH = os.path.join(os.path.dirname(_HERE), "tests", "golden", "replay_shapes.json")

_lib = None


def _load() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _ffi.load()                       # libreef_msm.so first (the replay library resolves it through its rpath as well)
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = ctypes.CDLL(LIB_PATH)
        lib.reef_replay_run.restype = ctypes.c_int
        lib.reef_replay_run.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
        lib.reef_replay_run_prove.restype = ctypes.c_int
        lib.reef_replay_run_prove.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        lib.reef_replay_check_selftest.restype = ctypes.c_int
        lib.reef_replay_check_selftest.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        lib.reef_replay_run_lookup.restype = ctypes.c_int
        lib.reef_replay_run_lookup.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        lib.reef_replay_lookup_selftest.restype = ctypes.c_int
        lib.reef_replay_lookup_selftest.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        lib.reef_replay_run_devices.restype = ctypes.c_int
        lib.reef_replay_run_devices.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_size_t,
                                                ctypes.c_char_p, ctypes.c_size_t]
        _lib = lib
    return _lib


def run(config: str = "cfg3", nofold: bool = True, tables: bool = False, shapes_path: str | None = None, devices=None) -> dict:
    """One replay; returns the harness's JSON line as a dict.  Raises on any failed call or mismatching commitment.
    devices: ordinals (may repeat) for the multi-device leg -- the final SNARK's arguments placed whole on per-device contexts and the
    document commitment through a device group (reef_msm_group_*), all from this one process; line["devices"] reports it."""
    buf = ctypes.create_string_buffer(32768)
    devs = list(devices or [])
    arr = (ctypes.c_int * max(len(devs), 1))(*devs)
    rc = _load().reef_replay_run_devices((shapes_path or SHAPES_PATH).encode(), config.encode(), int(nofold), int(tables), arr, len(devs), buf, len(buf))
    text = buf.value.decode(errors="replace")
    if rc != 0:
        raise RuntimeError(f"reef_replay_run({config}) failed with {rc}: {text}")
    return json.loads(text)


def shapes(shapes_path: str | None = None) -> dict:
    with open(shapes_path or SHAPES_PATH) as f:
        return {s["name"]: s for s in json.load(f)["shapes"]}


PROVE_PHASES = ("nifs", "spartan", "open", "hyrax")
LOOKUP_PHASES = ("lookup", "claim", "hyrax")


class ProofRejected(RuntimeError):
    """A check of the prove leg (.phase: nifs | spartan | open | hyrax) or of the lookup leg (lookup | claim | hyrax) failed."""

    def __init__(self, message: str, phase: str | None):
        super().__init__(message)
        self.phase = phase


def _phase_of(text: str):
    for p in PROVE_PHASES + LOOKUP_PHASES:
        if text.startswith(f"proof check failed [{p}]"):
            return p
    return None


def _prove(config: str, tamper: str | None, tables: bool, shapes_path: str | None, paired: bool) -> dict:
    if tamper is not None and tamper not in PROVE_PHASES:
        raise ValueError(f"tamper must be one of {PROVE_PHASES}")
    flags = " ".join(([f"tamper={tamper}"] if tamper else []) + (["tables"] if tables else []) + (["paired"] if paired else []))
    buf = ctypes.create_string_buffer(32768)
    rc = _load().reef_replay_run_prove((shapes_path or SHAPES_PATH).encode(), config.encode(), flags.encode(), buf, len(buf))
    text = buf.value.decode(errors="replace")
    if rc != 0:
        phase = _phase_of(text)
        if phase:
            raise ProofRejected(f"reef_replay_run_prove({config}): {text}", phase)
        raise RuntimeError(f"reef_replay_run_prove({config}) failed with {rc}: {text}")
    return json.loads(text)


def _run_prove(config: str = "cfg3", tamper: str | None = None, tables: bool = False, shapes_path: str | None = None) -> dict:
    """The prove leg: every device row of one proof (NIFS steps, the last fold, Spartan sum-checks and the batched opening on both
    curves, the Hyrax consistency argument) through the C ABI, then checked with the verifier's equations on the host.  Returns the
    JSON line as a dict.  A rejected proof raises ProofRejected naming the phase; tamper=<phase> alters one recorded value before
    the checks, so that it must.  One keyword-only option beside the four parameters (which tests/test_replay_prove_host.py pins):
    paired=True takes every step's comm_W and comm_T from one reef_nifs_commit_step and the first comm_W from reef_nifs_commit_running,
    and checks the folded instance's comm_W and comm_E from the device against the host's point operations; the line then carries
    "paired": true."""
    return _prove(config, tamper, tables, shapes_path, False)


@functools.wraps(_run_prove, assigned=("__module__", "__doc__", "__annotations__"))
def run_prove(config: str = "cfg3", tamper: str | None = None, tables: bool = False, shapes_path: str | None = None, *, paired: bool = False) -> dict:
    return _prove(config, tamper, tables, shapes_path, paired)


def check_selftest(tamper: str | None = None) -> dict:
    """The prove leg's checks on a tiny honest transcript made on the host (no GPU needed).  Returns the summary dict when every check
    accepts; raises ProofRejected naming the phase when one rejects (as it must with tamper=<phase>)."""
    buf = ctypes.create_string_buffer(4096)
    rc = _load().reef_replay_check_selftest(tamper.encode() if tamper else None, buf, len(buf))
    text = buf.value.decode(errors="replace")
    if rc == 1:
        raise ProofRejected(text, _phase_of(text))
    if rc != 0:
        raise RuntimeError(f"reef_replay_check_selftest failed with {rc}: {text}")
    return json.loads(text)


def run_lookup(config: str = "cfg3", mode: str | None = None, proj: int = 0, width: int = 1, tamper: str | None = None,
               shapes_path: str | None = None) -> dict:
    """The lookup leg: the lookup argument of every folding step as one chain of device rows -- the document's bytes through
    reef_doc_transform into device symbols, reef_hyrax_create / _commit and reef_sc_set_table_parts on that buffer, per step
    reef_sc_lookup and the N2 rounds under a stand-in transcript, the last running claim handed to reef_hyrax_eval_begin and its IPA --
    then checked on the host: every round's equations, T~ at the step's point recomputed outside the sum-check rows, the running claim
    from step to step, the claim against the evaluation the consistency argument proves, the Hyrax argument itself.  mode: "doc" |
    "hybrid" (None: from the shape); proj=k: nldoc over an aligned chunk of 2^(doc_log - k) symbols; width: bytes per device symbol.
    Returns the JSON line as a dict; a rejection raises ProofRejected with .phase in LOOKUP_PHASES (as it must with tamper=<phase>)."""
    if tamper is not None and tamper not in LOOKUP_PHASES:
        raise ValueError(f"tamper must be one of {LOOKUP_PHASES}")
    flags = ([f"mode={mode}"] if mode else []) + ([f"proj={int(proj)}"] if proj else []) + [f"width={int(width)}"] + ([f"tamper={tamper}"] if tamper else [])
    buf = ctypes.create_string_buffer(32768)
    rc = _load().reef_replay_run_lookup((shapes_path or SHAPES_PATH).encode(), config.encode(), " ".join(flags).encode(), buf, len(buf))
    text = buf.value.decode(errors="replace")
    if rc != 0:
        phase = _phase_of(text)
        if rc == 1 and phase in LOOKUP_PHASES:
            raise ProofRejected(f"reef_replay_run_lookup({config}): {text}", phase)
        raise RuntimeError(f"reef_replay_run_lookup({config}) failed with {rc}: {text}")
    return json.loads(text)


def lookup_selftest(tamper: str | None = None) -> dict:
    """The lookup leg's checks on a tiny honest transcript made on the host with plain loops (no GPU needed): ell = 4, 3 steps of 3
    lookups, mode doc and mode hybrid.  Returns the line as a dict -- both transcripts in full, canonical integers as hex strings --
    when every check accepts; raises ProofRejected naming the phase when one rejects (as it must with tamper=<phase>)."""
    buf = ctypes.create_string_buffer(65536)
    rc = _load().reef_replay_lookup_selftest(tamper.encode() if tamper else None, buf, len(buf))
    text = buf.value.decode(errors="replace")
    if rc == 1:
        raise ProofRejected(text, _phase_of(text))
    if rc != 0:
        raise RuntimeError(f"reef_replay_lookup_selftest failed with {rc}: {text}")
    return json.loads(text)
