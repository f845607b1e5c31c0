"""What a reset draws, bit for bit, against tests/golden/reset_draws.npz (tools/record_reset_draws.py wrote it on the commit before the reset
was cut into one piece per owner over one table of RNG streams).  One case per piece at B = 3 with set_env_offset(5): reset(seed=3), a second
reset on the same seed, an auto-reset after one step (reset_kernel) and three steps of myo_bench_rollout with episodes of one step (the same
reset body inside task_post_kernel), and after each the fields the piece writes.  Raw 32-bit words, no tolerance: the keys of every stream
(salt, id, counter layout) and the arithmetic on the draws are unchanged, so a word that differs is a draw taken from another stream."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_reset_draws as R  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "reset_draws.npz")) as z:
        return {k: z[k] for k in z.files}


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_fixture_covers_every_case_and_stage(golden):
    assert R.B == 3 and R.OFFSET == 5 and R.SEED == 3
    want = set()
    for case, (_, _, _, fields, skipped) in R.CASES.items():
        names = [n for f in fields for n in (("HFIELD_first", "HFIELD_last", "HFIELD_sum") if f == "HFIELD" else (f,))]
        want |= {f"{case}/{s}/{n}" for s in R.STAGES if s not in skipped for n in names}
    assert set(golden) == want
    # the record is of real draws: a drawn field is not constant over the envs, and the second episode differs from the first
    for case, field in (("pose_uniform_qpos", "QPOS"), ("stand_noise_clip", "QPOS"), ("walk_keyframe_noise", "QPOS"), ("terrain_rough", "HFIELD_first"),
                        ("fatigue_random", "FATIGUE"), ("hold_geom_size", "GEOMSIZE"), ("elbow_body_mass", "BODYMASS"), ("keyturn_body_offset", "BODYPOS"),
                        ("pen_body_quat", "BODYQUAT"), ("baoding_floored_target", "TARGET"), ("die_goal", "TARGET"), ("baoding_objects", "obj_mass"),
                        ("die_objects", "obj_size")):
        first, second = golden[f"{case}/reset/{field}"], golden[f"{case}/reset2/{field}"]
        assert not np.array_equal(first[0], first[1]) and not np.array_equal(first, second), (case, field)
    sign = np.concatenate([golden[f"baoding_floored_target/{s}/TARGET"][:, 1] for s in R.STAGES])
    assert set(sign) <= {-1.0, 0.0, 1.0} and len(set(sign)) > 1                                  # the floored component: a direction sign
    assert not golden["walk_sensor_rows/autoreset/SENSORDATA"].any() and not golden["walk_sensor_rows/autoreset/CFRC"].any()


@pytest.mark.parametrize("case", tuple(R.CASES))
def test_draws_equal_the_record(golden, case):
    got = R.draws(case)
    want = {k[len(case) + 1:]: v for k, v in golden.items() if k.startswith(case + "/")}
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, (case, k)
        differ = int((_words(got[k]) != _words(v)).sum())
        assert differ == 0, (case, k, differ)
