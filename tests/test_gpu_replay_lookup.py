"""The lookup leg of the replay on the device (`reef_replay cfgN lookup`, reef_amd/csrc/host/replay_lookup.hpp): the lookup argument of
every folding step as one chain of device rows -- bytes -> reef_doc_transform -> reef_hyrax_create / _commit and
reef_sc_set_table_parts on the same device buffer -> per step reef_sc_lookup and the N2 rounds -> the last running claim handed to
reef_hyrax_eval_begin and its IPA -- checked on the host by lookup_check.hpp.  Sizes: doc_log = 6 (fewer pairs than a wave in every
round), 11 (every round a posted one-launch round), 17 (the first rounds above the 2^14-pair bound of the posted rounds, then across
it; above the host bound of the table evaluation, so the document part comes from row N3)."""
import json

import pytest

from reef_amd import replay

pytestmark = pytest.mark.gpu

STEPS, LOOKUPS = 3, 5


def _shapes(tmp_path, doc_log, hybrid):
    """A shapes file in the format of tests/golden/replay_shapes.json with one shape of the given document size."""
    left = doc_log // 2
    shape = {"name": f"lk{doc_log}{'h' if hybrid else 'd'}", "w1": 1024, "c1": 1024, "w2": 1024, "c2": 1024, "steps": STEPS, "batch": LOOKUPS,
             "hyrax_row": 1 << (doc_log - left), "doc_log": doc_log, "symbol_bits": 8, "table_log": doc_log + (1 if hybrid else 0),
             "lookups": LOOKUPS, "merkle_log": 0}
    path = tmp_path / "shapes.json"
    path.write_text(json.dumps({"generated_by": "tests/test_gpu_replay_lookup.py", "shapes": [shape]}))
    return str(path), shape["name"]


def _accepted(line, doc_log, ell, mode, width, proj=0):
    assert line["leg"] == "lookup" and line["proof_checked"] is True
    assert (line["mode"], line["width"], line["proj"], line["doc_log"], line["table_log"]) == (mode, width, proj, doc_log, ell)
    assert line["rounds_checked"] == STEPS * ell and line["values_checked"] == STEPS * LOOKUPS
    assert line["consistency_rounds"] == doc_log - doc_log // 2
    assert line["table_eval"] == ("host" if ell <= 16 else "n3")
    assert line["points_checked"] >= 1 + 2 * line["consistency_rounds"]                 # comm_LZ and every L, R against their discrete logs


@pytest.mark.parametrize("doc_log", [6, 11, 17])
@pytest.mark.parametrize("width", [1, 2, 4])
def test_mode_doc_is_accepted(doc_log, width, tmp_path, gpu_lib):
    path, name = _shapes(tmp_path, doc_log, False)
    _accepted(replay.run_lookup(name, width=width, shapes_path=path), doc_log, doc_log, "doc", width)


@pytest.mark.parametrize("doc_log", [6, 11, 17])
def test_mode_hybrid_is_accepted(doc_log, tmp_path, gpu_lib):
    path, name = _shapes(tmp_path, doc_log, True)
    _accepted(replay.run_lookup(name, shapes_path=path), doc_log, doc_log + 1, "hybrid", 1)      # the mode comes from the shape


def test_a_projected_chunk_is_accepted(tmp_path, gpu_lib):
    path, name = _shapes(tmp_path, 11, False)
    _accepted(replay.run_lookup(name, proj=2, shapes_path=path), 11, 9, "doc", 1, proj=2)


@pytest.mark.parametrize("phase", replay.LOOKUP_PHASES)
@pytest.mark.parametrize("hybrid", [False, True], ids=["doc", "hybrid"])
def test_a_tampered_record_is_rejected_naming_the_phase(phase, hybrid, tmp_path, gpu_lib):
    path, name = _shapes(tmp_path, 11, hybrid)
    with pytest.raises(replay.ProofRejected) as e:
        replay.run_lookup(name, tamper=phase, shapes_path=path)
    assert e.value.phase == phase and f"proof check failed [{phase}]" in str(e.value)


def test_a_merkle_shape_is_a_usage_error(gpu_lib):
    with pytest.raises(RuntimeError, match="Merkle") as e:
        replay.run_lookup("cfg5")
    assert not isinstance(e.value, replay.ProofRejected)


def test_cfg3_from_the_golden_shapes_is_accepted(gpu_lib):
    line = replay.run_lookup("cfg3")
    shape = replay.shapes()["cfg3_1MiB_ascii_password"]
    assert line["proof_checked"] is True and line["mode"] == "doc" and line["table_eval"] == "n3"
    assert line["rounds_checked"] == shape["steps"] * shape["table_log"] and line["values_checked"] == shape["steps"] * shape["lookups"]
