"""CPU side of the bad-env contract (include/myo_hip.h, "A bad env"): the expectation itself -- the oracle's ABI twin, whose myoo_step1
resets like mj_sim_scene.py:54-61 -- goes through the sequence the GPU tests run on every kernel (tests/abi_backend.py::bad_env_scenario),
for the hand and the legs; and each assertion of tests/bad_env.py is shown to fire on rows that break it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_backend as A  # noqa: E402
import bad_env as BE  # noqa: E402
from myosuite_mjx_amd import capi  # noqa: E402

DEAD = (1, 6)


@pytest.fixture(scope="module")
def twin():
    return A.Backend(A.ORACLE_LIB, -1)


@pytest.mark.parametrize("kind", BE.KINDS)
@pytest.mark.parametrize("name", ["hand", "legs"])
def test_the_oracle_twin_keeps_the_contract(twin, request, name, kind):
    """Every injection kind raises the flag it is meant to raise on the oracle (nan_act / nan_ctrl: warning 2, a bad qacc), and the twin
    passes all four checks."""
    m = request.getfixturevalue(name)
    state = BE.hand_state(m, 8) if name == "hand" else BE.key_state(m, 8, 2)
    rec = A.bad_env_scenario(twin, m, state, kind, 10 if name == "hand" else 4, DEAD)
    assert (rec["flags"][list(DEAD)] == BE.FLAG_OF[kind]).all()
    assert rec["rows"][capi.F_TIME][0, 0] > 0


# ---- the assertions fire ---------------------------------------------------------------------------------------------------------------

def _good(B=4, nq=3, nu=2):
    rows = {capi.F_QPOS: np.full((B, nq), 0.5, np.float32), capi.F_QVEL: np.ones((B, nq), np.float32), capi.F_ACT: np.ones((B, nu), np.float32),
            capi.F_CTRL: np.ones((B, nu), np.float32), capi.F_WARMSTART: np.ones((B, nq), np.float32), capi.F_TIME: np.full((B, 1), 0.02, np.float32),
            capi.F_QACC: np.ones((B, nq), np.float32), capi.F_TENLEN: np.ones((B, nu), np.float32), capi.F_ACTFORCE: np.ones((B, nu), np.float32),
            capi.F_DIAG: np.ones((B, 8), np.int32)}
    qpos0 = np.array([0.1, 0.2, 0.3], np.float32)
    rows[capi.F_QPOS][1] = qpos0
    for f in BE.ZERO:
        if f in rows:
            rows[f][1] = 0
    return rows, np.array([0, 1, 0, 4], np.int32), qpos0


def test_reset_exact_fires():
    rows, flags, qpos0 = _good()
    BE.assert_reset_exact(rows, flags, (1,), qpos0, capi.FLAG_BAD_STATE)
    for f in (capi.F_QPOS, capi.F_QACC, capi.F_WARMSTART, capi.F_TENLEN, capi.F_ACTFORCE, capi.F_TIME, capi.F_CTRL):
        r = {k: x.copy() for k, x in rows.items()}
        r[f][1, 0] += np.float32(1e-7) if f != capi.F_QPOS else np.float32(1e-6)
        with pytest.raises(AssertionError):
            BE.assert_reset_exact(r, flags, (1,), qpos0, capi.FLAG_BAD_STATE)
    with pytest.raises(AssertionError):      # the other flag
        BE.assert_reset_exact(rows, flags, (1,), qpos0, capi.FLAG_BAD_QACC)
    with pytest.raises(AssertionError):      # both flags
        BE.assert_reset_exact(rows, np.array([0, 3, 0, 0], np.int32), (1,), qpos0, capi.FLAG_BAD_STATE)
    with pytest.raises(AssertionError):      # a flag on a neighbour
        BE.assert_reset_exact(rows, np.array([0, 1, 2, 0], np.int32), (1,), qpos0, capi.FLAG_BAD_STATE)


def test_finite_and_neighbours_fire():
    rows, _, _ = _good()
    BE.assert_all_fields_finite(rows)
    BE.assert_neighbours_bitwise(rows, {k: x.copy() for k, x in rows.items()}, (1,))
    for v in (np.nan, np.inf):
        r = {k: x.copy() for k, x in rows.items()}
        r[capi.F_ACTFORCE][3, 1] = v
        with pytest.raises(AssertionError, match="F_ACTFORCE"):
            BE.assert_all_fields_finite(r)
    c = {k: x.copy() for k, x in rows.items()}
    c[capi.F_QPOS][1] += 1                     # the bad env itself may differ
    BE.assert_neighbours_bitwise(rows, c, (1,))
    c[capi.F_QACC][2, 0] = np.nextafter(np.float32(1), np.float32(2))
    with pytest.raises(AssertionError, match="F_QACC"):
        BE.assert_neighbours_bitwise(rows, c, (1,))
    c = {k: x.copy() for k, x in rows.items()}
    c[capi.F_DIAG][0, 2] = 7
    with pytest.raises(AssertionError, match="F_DIAG"):
        BE.assert_neighbours_bitwise(rows, c, (1,))
    z = {k: x.copy() for k, x in rows.items()}
    z[capi.F_QVEL][0, 0] = -0.0               # bitwise, not numerically equal
    r = {k: x.copy() for k, x in rows.items()}
    r[capi.F_QVEL][0, 0] = 0.0
    with pytest.raises(AssertionError, match="F_QVEL"):
        BE.assert_neighbours_bitwise(r, z, (1,))


class _Fake:
    """A batch whose step adds its hidden residue to qvel: what a stale warm start does."""

    def __init__(self, rows, residue=0.0):
        self.rows, self.residue = {k: x.copy() for k, x in rows.items()}, residue

    def write(self, f, a):
        self.rows[f] = np.array(a, copy=True)

    def read(self, f):
        return self.rows.get(f)

    def step(self, nsub):
        self.rows[capi.F_QVEL] = self.rows[capi.F_QVEL] + np.float32(1) + np.float32(self.residue)

    def status(self):
        return np.zeros(len(self.rows[capi.F_QPOS]), np.int32)


def test_no_residue_fires():
    rows, _, qpos0 = _good()
    BE.assert_no_residue(_Fake(rows), _Fake(rows), rows, (1,), qpos0, 1, rows[capi.F_CTRL])
    with pytest.raises(AssertionError, match="F_QVEL"):
        BE.assert_no_residue(_Fake(rows, 1e-6), _Fake(rows), rows, (1,), qpos0, 1, rows[capi.F_CTRL])
    stale = {k: x.copy() for k, x in rows.items()}
    stale[capi.F_QVEL][1, 0] = 1e-6           # a state row of the bad env that is not the reset state: the fresh batch starts from zero
    with pytest.raises(AssertionError, match="F_QVEL"):
        BE.assert_no_residue(_Fake(stale), _Fake(rows), stale, (1,), qpos0, 1, rows[capi.F_CTRL])


def test_inject_makes_one_entry_per_bad_env_bad():
    st = {capi.F_QPOS: np.zeros((8, 5), np.float32), capi.F_QVEL: np.zeros((8, 5), np.float32), capi.F_ACT: np.zeros((8, 4), np.float32),
          capi.F_CTRL: np.zeros((8, 4), np.float32)}
    for kind in BE.KINDS:
        out = BE.inject(kind, st, DEAD)
        f, v = BE._WHERE[kind]
        for g in st:
            badrows = np.unique(np.argwhere(~(np.abs(out[g]) < 1e10))[:, 0]).tolist()
            assert badrows == (list(DEAD) if g == f else []), (kind, g)
        assert not st[f].any()
