"""The prove leg of the replay on the device (`reef_replay cfgN prove`, reef_amd.replay.run_prove): every device row of one proof --
the NIFS step per folding step and curve (3f), the last fold, the Spartan sum-checks (3g) and the batched IPA opening (3h) on both
curves on the instance the folds left on the device, the Hyrax consistency argument over the committed document (3i) -- driven
through the provider mirror in the call order of INTEGRATION.md 2f-2i, then checked with the verifier's equations on the host and
every returned point against its discrete logarithm.  The matrices are synthetic R1CS of the shapes' sizes
(tests/golden/replay_shapes.json)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pow2(n: int) -> int:
    return 1 << (n - 1).bit_length()


def _shape(cfg):
    from reef_amd import replay
    return next(s for name, s in replay.shapes().items() if cfg in name)


def _check_line(line, shape):
    assert line["replay"] == shape["name"] and line["leg"] == "prove" and line["proof_checked"] is True
    assert (line["w1"], line["c1"], line["w2"], line["c2"]) == (shape["w1"], shape["c1"], shape["w2"], shape["c2"])
    assert "SYNTHETIC" in line["matrices"] and "stand-in" in line["transcript"]
    for cv, w, c in (("pallas", shape["w1"], shape["c1"]), ("vesta", shape["w2"], shape["c2"])):
        ncp, nvp = _pow2(c), _pow2(w)
        assert (line[f"num_cons_pad_{cv}"], line[f"num_vars_pad_{cv}"], line[f"pad_{cv}"]) == (ncp, nvp, max(ncp, nvp))
        assert line[f"outer_rounds_{cv}"] == ncp.bit_length() - 1                 # log2(num_cons_pad) cubic rounds
        assert line[f"inner_rounds_{cv}"] == (2 * nvp).bit_length() - 1           # over z's 2 num_vars_pad entries
        assert line[f"ipa_rounds_{cv}"] == max(ncp, nvp).bit_length() - 1
        assert line[f"spartan_ms_{cv}"] > 0 and line[f"open_ms_{cv}"] > 0
        assert line[f"nnz_{cv}"] > 3 * c
    assert line["steps"] == shape["steps"] and len(line["step_ms"]) == shape["steps"]
    assert line["ms_per_step"] > 0 and line["final_fold_ms"] > 0 and line["nifs_ms_per_step"] > 0
    # every commitment of the steps (comm_W, comm_T per curve), the first instances, the last fold, and 2 points per IPA round
    expected = 2 + 4 * shape["steps"] + 2 + 2 * (line["ipa_rounds_pallas"] + line["ipa_rounds_vesta"])
    if shape["doc_log"]:
        left = shape["doc_log"] // 2
        assert line["doc_log"] == shape["doc_log"] and line["hyrax_left"] == left
        assert line["consistency_rounds"] == shape["doc_log"] - left and line["consistency_ms"] > 0
        expected += 2 + 1 + 2 * line["consistency_rounds"]                          # two row commitments, comm_LZ, L and R per round
    else:
        assert line["consistency_rounds"] == 0 and line["consistency_ms"] == 0
    assert line["points_checked"] == expected
    parts = (line["nifs_init_ms"] + line["ms_per_step"] * shape["steps"] + line["final_fold_ms"] + line["spartan_ms_pallas"] + line["spartan_ms_vesta"]
             + line["open_ms_pallas"] + line["open_ms_vesta"] + line["consistency_ms"])
    assert abs(line["total_prove_device_ms"] - parts) < 1e-2


@pytest.mark.parametrize("cfg", ["cfg1", "cfg3", "cfg4"])
def test_prove_leg_passes_every_check(cfg, gpu_lib):
    from reef_amd import replay
    _check_line(replay.run_prove(cfg), _shape(cfg))


@pytest.mark.parametrize("phase", ["nifs", "spartan", "open", "hyrax"])
def test_a_tampered_record_fails_naming_its_phase(phase, gpu_lib):
    from reef_amd import replay
    with pytest.raises(replay.ProofRejected) as e:
        replay.run_prove("cfg1", tamper=phase)
    assert e.value.phase == phase and f"[{phase}]" in str(e.value)


def test_prove_leg_cfg5_merkle(gpu_lib):
    """BASELINE configs[4]: a 2^20-constraint primary circuit, no Hyrax document (--merkle).  The slow one: about 10^7 matrix entries in
    the host checks."""
    from reef_amd import replay
    _check_line(replay.run_prove("cfg5"), _shape("cfg5"))


def test_the_executable_prints_one_checked_line(gpu_lib):
    exe = os.path.join(ROOT, "reef_amd", "_lib", "reef_replay")
    out = subprocess.run([exe, "cfg1", "prove"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1 and '"proof_checked": true' in lines[0]
    bad = subprocess.run([exe, "cfg1", "prove", "tamper=spartan"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1 and "proof check failed [spartan]" in bad.stderr
