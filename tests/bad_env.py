"""What the bad-env tests share (include/myo_hip.h, "A bad env"): the ways an env is made bad, and the checks of what the launch leaves
behind, as plain functions that assert on rows read back -- {field id: [B, width] array}, from whichever backend.  A `batch` here is
anything with write(field, rows), read(field) (None where the batch has no such field), step(nsub) and status(): tests/abi_backend.py's
AbiBatch on the HIP library or on the oracle's CPU twin, or HipRows around a capi.HipBatch with a task configured.
tests/test_bad_env_host.py runs the bare sequence on the CPU twin and shows on synthetic rows that each assertion fires;
tests/test_gpu_bad_env.py runs it on every step kernel and task."""
import numpy as np

from myosuite_mjx_amd import capi

# ---- injection kinds: all through myo_batch_write (nan_action: through the action buffer, see the task tests).  The first three make the
# state bad at the start of substep 0.  nan_act: a finite state whose substep-0 qacc is bad.  nan_ctrl (MYO_ACTMAP_NONE): the control only
# drives the activation derivative, so substep 0 is clean, the activation is NaN after it and the qacc of substep 1 is bad -- the one kind
# whose env goes bad in the middle of a launch, which tells "reset and stop" from "reset and carry on"
KINDS = ("nan_qvel", "huge_qvel", "nan_act", "nan_ctrl", "nan_qpos")
FLAG_OF = {"nan_qvel": capi.FLAG_BAD_STATE, "huge_qvel": capi.FLAG_BAD_STATE, "nan_qpos": capi.FLAG_BAD_STATE,
           "nan_act": capi.FLAG_BAD_QACC, "nan_ctrl": capi.FLAG_BAD_QACC, "nan_action": capi.FLAG_BAD_QACC}
_WHERE = {"nan_qvel": (capi.F_QVEL, np.nan), "huge_qvel": (capi.F_QVEL, 1e12), "nan_qpos": (capi.F_QPOS, np.nan), "nan_act": (capi.F_ACT, np.nan),
          "nan_ctrl": (capi.F_CTRL, np.nan), "nan_action": (capi.F_ACTION, np.nan)}

STATE = (capi.F_QPOS, capi.F_QVEL, capi.F_ACT, capi.F_CTRL, capi.F_WARMSTART, capi.F_TIME)            # what a launch starts from
ZERO = (capi.F_QVEL, capi.F_ACT, capi.F_CTRL, capi.F_WARMSTART, capi.F_QACC, capi.F_TIME,             # exactly zero in a bad env after the launch
        capi.F_TENLEN, capi.F_ACTFORCE, capi.F_LINKX, capi.F_SENSORDATA, capi.F_CFRC)
# every field a launch or an observation pass writes (inputs -- action buffer, terrain, overrides, targets -- are not outputs)
OUTPUTS = STATE + (capi.F_OBS, capi.F_REWARD, capi.F_DONE, capi.F_SOLVED, capi.F_FLAGS, capi.F_DIAG, capi.F_QACC, capi.F_TENLEN, capi.F_ACTFORCE,
                   capi.F_SITEXPOS, capi.F_ELAPSED, capi.F_FATIGUE, capi.F_LINKX, capi.F_METRICS, capi.F_SENSORDATA, capi.F_CFRC)
NAME = {getattr(capi, n): n for n in dir(capi) if n.startswith("F_") and n != "F_COUNT"}


class HipRows:
    """A capi.HipBatch as a `batch` of this module; step = the callable the case gives (action map, fused passes, observation)."""

    def __init__(self, b, step):
        self.b, self._step = b, step

    def write(self, field, a):
        self.b.write(field, a)

    def read(self, field):
        try:
            return self.b.read(field)
        except capi.MyoError:
            return None

    def step(self, nsub):
        self._step(self.b, nsub)

    def status(self):
        return self.b.status()


def inject(kind, state, dead):
    """A copy of `state` ({field: rows}) with one entry of each env in `dead` made bad; the entry differs from env to env."""
    f, v = _WHERE[kind]
    out = {k: np.array(x, np.float32, copy=True) for k, x in state.items()}
    for e in dead:
        out[f][e, (3 + 5 * e) % out[f].shape[1]] = v
    return out


def read_all(batch):
    """Every output field the batch answers for."""
    rows = {f: batch.read(f) for f in OUTPUTS}
    return {f: x for f, x in rows.items() if x is not None}


# ---- assertions ------------------------------------------------------------------------------------------------------------------------

def assert_reset_exact(rows, flags, dead, qpos0, flag):
    """The bad envs hold the reset state exactly and carry `flag`; nobody else carries a bad-env flag."""
    bad_bits = capi.FLAG_BAD_STATE | capi.FLAG_BAD_QACC
    for e in range(len(flags)):
        if e in dead:
            assert flags[e] & bad_bits == flag, (e, int(flags[e]), flag)
        else:
            assert flags[e] & bad_bits == 0, (e, int(flags[e]))
    for e in dead:
        assert np.array_equal(rows[capi.F_QPOS][e], np.asarray(qpos0, np.float32)), (e, "F_QPOS")
        for f in ZERO:
            if f in rows:
                assert not rows[f][e].any() and np.isfinite(rows[f][e]).all(), (e, NAME[f], rows[f][e][:8])


def assert_all_fields_finite(rows):
    for f, x in rows.items():
        if f not in capi.INT_FIELDS:
            assert np.isfinite(x).all(), (NAME[f], np.argwhere(~np.isfinite(x))[:4].tolist())


def assert_neighbours_bitwise(rows, rows_clean, dead):
    """The same launch with and without the injection: every field of every other env is the same, bit for bit."""
    keep = [e for e in range(len(rows[capi.F_QPOS])) if e not in dead]
    assert set(rows) == set(rows_clean)
    for f in rows:
        assert rows[f][keep].tobytes() == rows_clean[f][keep].tobytes(), NAME[f]


def reset_rows(rows, dead, reset_qpos):
    """The launch state of a fresh batch for the residue check: `rows` with the reset state written out for the envs in `dead`."""
    st = {f: rows[f].copy() for f in STATE}
    for e in dead:
        st[capi.F_QPOS][e] = reset_qpos
        for f in STATE[1:]:
            st[f][e] = 0
    return st


def assert_no_residue(batch, fresh, rows, dead, reset_qpos, nsub, ctrl=None, fields=STATE + (capi.F_QACC,), f64_state=False):
    """Two more env steps with finite controls: the formerly bad envs step exactly like envs of `fresh`, a batch that never saw the
    injection and is written with the reset state (and the step counters of `batch`).  Anything a bad env leaves behind outside its state
    rows -- a warm start, a warm-start table, a mark, a cost word -- shows up here.  f64_state: the backend keeps its state in float64 (the
    CPU twin), where a qpos0 that came through a float32 write is not the qpos0 of a reset: `batch` gets the same float32 rows written."""
    st = reset_rows(rows, dead, reset_qpos)
    if ctrl is not None:
        st[capi.F_CTRL] = ctrl
        batch.write(capi.F_CTRL, ctrl)
    for f, x in st.items():
        fresh.write(f, x)
        if f64_state:
            batch.write(f, x)
    if capi.F_ELAPSED in rows:
        fresh.write(capi.F_ELAPSED, rows[capi.F_ELAPSED])
    for _ in range(2):
        batch.step(nsub)
        fresh.step(nsub)
    a, b = read_all(batch), read_all(fresh)
    for f in fields:
        if f in a:
            for e in dead:
                assert a[f][e].tobytes() == b[f][e].tobytes(), (e, NAME[f])
    assert_all_fields_finite(a)
    assert not (batch.status()[list(dead)] & (capi.FLAG_BAD_STATE | capi.FLAG_BAD_QACC)).any()
    return a, b


def run_bare(batch, clean, fresh, model, state, kind, nsub, dead, f64_state=False):
    """The bare-step contract for one injection kind: `batch` gets the injected state, `clean` the state as it is, both step one env step;
    then all four checks.  Returns the rows and flags read on the way."""
    for b, st in ((batch, inject(kind, state, dead)), (clean, state)):
        for f, x in st.items():
            b.write(f, x)
        b.step(nsub)
    rows, rows_clean, flags = read_all(batch), read_all(clean), batch.status()
    assert not (clean.status() & (capi.FLAG_BAD_STATE | capi.FLAG_BAD_QACC)).any()
    assert_reset_exact(rows, flags, dead, model.qpos0, FLAG_OF[kind])
    assert_all_fields_finite(rows)
    assert_neighbours_bitwise(rows, rows_clean, dead)
    ctrl = np.random.default_rng(11).uniform(0, 1, state[capi.F_CTRL].shape).astype(np.float32)
    after, after_fresh = assert_no_residue(batch, fresh, rows, dead, model.qpos0, nsub, ctrl, f64_state=f64_state)
    return dict(rows=rows, rows_clean=rows_clean, flags=flags, after=after, after_fresh=after_fresh)


def hand_state(m, B, seed=15, spread=0.4):
    """B states of a hinge-only model (the hand): joints within `spread` of their range, moving, muscles part activated."""
    rng = np.random.default_rng(seed)
    lo, hi = m.jnt_range[:, 0], m.jnt_range[:, 1]
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    f32 = np.float32
    return {capi.F_QPOS: (mid + spread * half * rng.uniform(-1, 1, (B, m.nq))).astype(f32), capi.F_QVEL: rng.normal(0, 0.5, (B, m.nv)).astype(f32),
            capi.F_ACT: rng.uniform(0, 1, (B, m.nu)).astype(f32), capi.F_CTRL: rng.uniform(0, 1, (B, m.nu)).astype(f32)}


def key_state(m, B, key, seed=15):
    """B states around keyframe `key` of a model with keyframes (legs: 2 = walking, feet on the ground; objects: 0), small joint noise on
    the hinges after a free root, slow, muscles part activated."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    q = np.tile(np.asarray(m.key_qpos, float).reshape(-1, m.nq)[key], (B, 1))
    if m.nq == m.nv + 1:
        q[:, 7:] += rng.normal(0, 0.02, (B, m.nq - 7))
    return {capi.F_QPOS: q.astype(f32), capi.F_QVEL: rng.normal(0, 0.1, (B, m.nv)).astype(f32),
            capi.F_ACT: rng.uniform(0, 0.5, (B, m.nu)).astype(f32), capi.F_CTRL: rng.uniform(0, 0.5, (B, m.nu)).astype(f32)}


# ---- tasks -----------------------------------------------------------------------------------------------------------------------------

TASK_ROWS = (capi.F_OBS, capi.F_REWARD, capi.F_DONE, capi.F_SOLVED, capi.F_SITEXPOS)


def task_contained(env, clean, kind, dead, flag="kind", fused_obs=False, seed=0):
    """A task whose observation is a pass of its own (fused_obs: the walk / stand pass inside the step launch).  `env` and `clean` are two
    envs of one id after the same reset.  One env step with env `dead` made bad by `kind` (nan_action: a NaN in its action): every row is
    finite, the other envs' rows are those of `clean` bit for bit, the bad env holds the reset state with `flag` (None: the action map
    clips the NaN away and nobody is bad), its step counter counts on, and its task rows are bit for bit what the observation pass
    writes for the reset state at the step count the pass saw.  Returns the rows of `env` and the flags."""
    m, b = env.mjmodel, env.batch
    B, D = b.B, (dead,)
    a = np.random.default_rng(seed).uniform(-1, 1, (B, m.nu)).astype(np.float32)
    a_bad = a
    if kind == "nan_action":
        a_bad = inject(kind, {capi.F_ACTION: a}, D)[capi.F_ACTION]
    else:
        st = {f: b.read(f) for f in (capi.F_QPOS, capi.F_QVEL, capi.F_ACT, capi.F_CTRL)}
        f = _WHERE[kind][0]
        b.write(f, inject(kind, st, D)[f])
    env.step(a_bad)
    clean.step(a)
    rows, rows_clean, flags = read_all(HipRows(b, None)), read_all(HipRows(clean.batch, None)), env.status()
    bad_bits = capi.FLAG_BAD_STATE | capi.FLAG_BAD_QACC
    assert not (clean.status() & bad_bits).any()
    assert_all_fields_finite(rows)
    assert_neighbours_bitwise(rows, rows_clean, D)
    if flag is None:
        assert not (flags & bad_bits).any()
        return rows, flags
    assert_reset_exact(rows, flags, D, m.qpos0, FLAG_OF[kind] if flag == "kind" else flag)
    assert np.array_equal(rows[capi.F_ELAPSED], rows_clean[capi.F_ELAPSED])          # sim.reset() does not end the gym episode
    for f, x in reset_rows(rows_clean, D, m.qpos0).items():
        clean.batch.write(f, x)
    if fused_obs:      # the fused pass runs before the launch counts the step
        clean.batch.write(capi.F_ELAPSED, rows_clean[capi.F_ELAPSED] - 1)
    clean.batch.obs()
    for f in TASK_ROWS:
        assert rows[f][dead].tobytes() == clean.batch.read(f)[dead].tobytes(), NAME[f]
    return rows, flags
