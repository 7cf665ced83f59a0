"""The prove leg of the replay ends with the verifier's device work (`reef_replay cfgN prove`, reef_amd.replay.run_prove): after the host
checks pass, reef_spartan_eval_matrices (include/reef_msm.h 3k) runs on both curves' contexts at the recorded (r_x, r_y), and
A~ + r B~ + r^2 C~ must equal the recorded claims_inner[0] and the host's own value; then reef_ipa_check_eq (3j) must accept each recorded
opening.  The line carries the times of both, and of the host loop the first replaces."""
import pytest

pytestmark = pytest.mark.gpu


def test_the_prove_leg_is_verified_on_the_device(gpu_lib):
    from reef_amd import replay
    line = replay.run_prove("cfg1")
    assert line["proof_checked"] is True and line["device_verified"] is True
    for cv in ("pallas", "vesta"):
        assert line[f"verify_evals_ms_{cv}"] > 0 and line[f"verify_evals_host_ms_{cv}"] > 0
        assert line[f"verify_ipa_ms_{cv}"] > 0
    parts = (line["nifs_init_ms"] + sum(line["step_ms"]) + line["final_fold_ms"] + line["spartan_ms_pallas"] + line["spartan_ms_vesta"] +
             line["open_ms_pallas"] + line["open_ms_vesta"] + line["consistency_ms"])
    assert abs(line["total_prove_device_ms"] - parts) < 1e-2          # the verifier's time is not the prover's
