"""The canonical rows of every task, bit for bit, against tests/golden/task_rows.npz (tools/record_task_rows.py wrote it on the commit
before the row layouts moved into one record per task).  One id per task at B = 3, reset(seed=0) and three steps, once plain and once
with rwd_dict=True (the two reward branches of each observation body): MYO_F_OBS, reward, done and solved after the reset and after the
last step, and the reward-term row in the second run.  Equality, no tolerance: a layout change moves integer index arithmetic only, so a
float that differs is a block written to, or read from, the wrong place."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_task_rows as R  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "task_rows.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_covers_every_task_in_both_modes(golden):
    import test_gpu_obs_terms as T
    from myosuite_mjx_amd import envs
    assert R.IDS == T.IDS and R.B == 3 and R.STEPS == T.STEPS
    assert set(envs.REGISTRY[i]["task"] for i in R.IDS) == set(s["task"] for s in envs.REGISTRY.values()) - {"track"}
    whats = {"plain": ("obs", "reward", "done", "solved"), "rwd": ("obs", "reward", "done", "solved", "rwd")}
    assert sorted(golden) == sorted(f"{i}/{m}/{when}/{w}" for i in R.IDS for m in whats for when in ("reset", "last") for w in whats[m])
    for i in R.IDS:                                                           # the rows are real: finite, moving, and rewarded
        assert np.isfinite(golden[f"{i}/plain/last/obs"]).all() and np.abs(golden[f"{i}/plain/last/obs"]).max() > 0
        assert not np.array_equal(golden[f"{i}/plain/last/obs"], golden[f"{i}/plain/reset/obs"])
        assert np.abs(golden[f"{i}/plain/last/reward"]).max() > 0 and np.abs(golden[f"{i}/rwd/last/rwd"]).max() > 0


@pytest.mark.parametrize("mode", tuple(R.MODES))
@pytest.mark.parametrize("env_id", R.IDS)
def test_rows_equal_the_record(golden, env_id, mode):
    got = R.rows(env_id, mode)
    want = {k[len(env_id) + len(mode) + 2:]: v for k, v in golden.items() if k.startswith(f"{env_id}/{mode}/")}
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape and np.array_equal(got[k], v, equal_nan=True), (env_id, mode, k)
