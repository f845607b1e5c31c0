"""The shared checks of tests/hand_task_checks.py that only GPU tests call, on synthetic arrays and a stub env (no GPU, no library):
their assertions fire when they should."""
import numpy as np
import pytest

import hand_task_checks as H

B = 4096


def test_assert_uniform_passes_on_uniform_and_fires_on_half_the_range():
    x = np.random.default_rng(0).uniform(-1, 1, B)
    H.assert_uniform(x, -1, 1)
    with pytest.raises(AssertionError):
        H.assert_uniform(np.clip(x, -1, 0), -1, 1)


class StubEnv:
    """Draws a pure function of (seed, global env id), as the device RNG's are; `shift` moves the ids of every shard but the first."""

    def __init__(self, n, seed, off, shift):
        self.ids, self.seed = np.arange(off + (shift if off else 0), off + (shift if off else 0) + n), seed

    def reset(self, seed=None):
        self.seed = self.seed if seed is None else seed
        self.draws = np.sin(self.ids * 12.9898 + self.seed * 78.233) * 43758.5453 % 1


@pytest.mark.parametrize("shift", [0, 1])
def test_assert_deterministic_and_sharded(shift):
    def make_env(n, seed, off):
        return StubEnv(n, seed, off, shift)

    whole = make_env(B, H.SEED, 0)
    whole.reset()
    if shift == 0:
        H.assert_deterministic_and_sharded(make_env, lambda e: (e.draws,), B, (whole.draws,))
    else:
        with pytest.raises(AssertionError, match=str(B // 2)):         # the shard at env_offset B // 2, one env off
            H.assert_deterministic_and_sharded(make_env, lambda e: (e.draws,), B, (whole.draws,))


def test_deterministic_fires_when_the_seed_is_ignored():
    class Deaf(StubEnv):
        def reset(self, seed=None):
            StubEnv.reset(self, H.SEED)

    whole = Deaf(B, H.SEED, 0, 0)
    whole.reset()
    with pytest.raises(AssertionError):
        H.assert_deterministic_and_sharded(lambda n, seed, off: Deaf(n, seed, off, 0), lambda e: (e.draws,), B, (whole.draws,))


def test_same_contacts_leaves_out_flagged_envs_and_other_contact_counts():
    flags = np.array([0, 4, 0, 0], np.int32)
    ncon, ncon_oracle = np.array([3, 3, 2, 0], np.int32), np.array([3, 3, 3, 0])
    assert H.same_contacts(flags, ncon, ncon_oracle).tolist() == [True, False, False, True]
