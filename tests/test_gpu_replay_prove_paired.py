"""The prove leg with `paired` (`reef_replay cfgN prove paired`, replay.run_prove(.., paired=True)): every step's comm_W and comm_T
from one reef_nifs_commit_step, the first comm_W from reef_nifs_commit_running, and after the last fold the device's comm_W and comm_E
of the folded instance against the host's tracked point operations.  Without the flag the line is the default leg's."""
import pytest

pytestmark = pytest.mark.gpu


def test_paired_prove_leg_passes_every_check_and_says_so(gpu_lib):
    from reef_amd import replay
    line = replay.run_prove("cfg1", paired=True)
    assert line["proof_checked"] is True and line["device_verified"] is True and line["paired"] is True
    default = replay.run_prove("cfg1")
    assert "paired" not in default
    assert default["proof_checked"] is True and default["device_verified"] is True
    # the same points and four more: comm_W and comm_E of the folded instance per curve, from reef_nifs_commit_running
    assert line["points_checked"] == default["points_checked"] + 4
