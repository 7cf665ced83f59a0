"""The verifier's half of the lookup leg's consistency argument on the device (reef_amd/csrc/host/replay_lookup.hpp): a vk built from
the rows reef_hyrax_commit produced (reef_hyrax_vk_create), comm_LZ through it (reef_hyrax_vk_comm_lz) equal to the prover's
reef_hyrax_eval_comm_own, and reef_ipa_check_eq accepting the proof against it."""
import pytest

from reef_amd import replay

pytestmark = pytest.mark.gpu


def test_cfg3_is_verified_on_the_device(gpu_lib):
    line = replay.run_lookup("cfg3")
    assert line["proof_checked"] is True and line["device_verified"] is True
    assert line["verify_comm_lz_ms"] > 0 and line["verify_ipa_ms"] > 0
