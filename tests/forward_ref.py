"""The float64 side of the forward-pass checks (tests/test_forward_host.py, tests/test_gpu_forward.py): the oracle's own forward pass at a
given qpos -- body, geom and site frames and the contact list -- plus site_xmat, which the oracle does not keep, restated from its body
frames; the float32 oracle's deviation from it, which sets the bounds of the contact geometry; and the matching of two contact lists."""
import numpy as np

FRAME_FIELDS = ("xpos", "xmat", "xipos", "geom_xpos", "geom_xmat", "site_xpos")


def quat2mat(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def oracle_forward(o, m, qpos, hfield=None):
    """Frames and contacts of oracle `o` (a model `m`) at qpos: {xpos [nb, 3], xmat [nb, 3, 3], xipos, geom_xpos, geom_xmat, site_xpos,
    site_xmat (None without site_quat), contacts [n, 9] = dist, pos, normal, geom1, geom2}."""
    o.reset()
    if hfield is not None:
        o.set_hfield(hfield)
    o.set_state(qpos=qpos)
    o.forward()
    out = {}
    for f in FRAME_FIELDS:
        a = np.array(o.field(f), np.float64)
        out[f] = a.reshape(-1, 3, 3) if f.endswith("mat") else a.reshape(-1, 3)
    out["site_xmat"] = None
    if "site_quat" in m.arrays:
        out["site_xmat"] = np.array([out["xmat"][b] @ quat2mat(q) for b, q in zip(m.site_bodyid, m.site_quat)]).reshape(-1, 3, 3)
    out["contacts"] = np.array(o.contacts(), np.float64).reshape(-1, 9)
    return out


def pair_multiset(con):
    """Sorted list of (geom1, geom2) of a contact array [n, >= 9] (oracle layout) or of (geom1, geom2) columns."""
    return sorted((int(c[7]), int(c[8])) for c in con)


def gpu_contacts(rec, ncon, e):
    """Env e's contacts of a FWD_CONTACT host array in the oracle's layout [n, 9] (dist, pos, normal, geom1, geom2), and its frames [n, 3, 3]."""
    r = rec[e, :int(ncon[e])]
    ids = r[:, 13:16].copy().view(np.int32)
    con = np.concatenate([r[:, 0:7].astype(np.float64), ids[:, 0:2].astype(np.float64)], axis=1)
    return con, r[:, 4:13].astype(np.float64).reshape(-1, 3, 3)


def match_contacts(a, b):
    """For two contact arrays [n, 9] with the same pair multiset: index arrays (ia, ib) that put them in the same order -- by pair, and
    the several contacts of one pair (the two of a plane - capsule or plane - cylinder pair, the prisms under one foot geom) sorted by
    position in `a` and given their nearest partner by position in `b`."""
    ia, ib = [], []
    pa, pb = [(int(r[7]), int(r[8])) for r in a], [(int(r[7]), int(r[8])) for r in b]
    for p in sorted(set(pa)):
        ga = sorted((i for i in range(len(a)) if pa[i] == p), key=lambda i: tuple(a[i, 1:4]))
        gb = [i for i in range(len(b)) if pb[i] == p]
        for i in ga:
            j = min(gb, key=lambda j: float(np.sum((b[j, 1:4] - a[i, 1:4]) ** 2)))
            gb.remove(j)
            ia.append(i); ib.append(j)
    return np.array(ia, int), np.array(ib, int)


def deviation(a, b):
    """max |dist|, |pos|, |normal| difference of two contact arrays with equal pair multisets, matched per pair."""
    if len(a) == 0:
        return np.zeros(3)
    ia, ib = match_contacts(a, b)
    d = np.abs(a[ia][:, :7] - b[ib][:, :7])
    return np.array([d[:, 0].max(), d[:, 1:4].max(), d[:, 4:7].max()])


def worst_contacts(a, b, k=3):
    """The k contacts of b that lie farthest from their partner in a, as text: pair, |d dist|, |d pos|, its part along the normal, |d normal|."""
    if len(a) == 0:
        return ""
    ia, ib = match_contacts(a, b)
    rows = []
    for i, j in zip(ia, ib):
        dp = b[j, 1:4] - a[i, 1:4]
        rows.append((np.abs(dp).max(), f"({int(a[i, 7])}, {int(a[i, 8])}) d dist {abs(b[j, 0] - a[i, 0]):.1e} d pos {np.abs(dp).max():.1e} (along the normal {abs(dp @ a[i, 4:7]):.1e}) "
                                       f"d normal {np.abs(b[j, 4:7] - a[i, 4:7]).max():.1e}"))
    return "; ".join(t for _, t in sorted(rows, reverse=True)[:k])


FLOORS = np.array([5e-6, 5e-6, 1e-5])      # dist, pos, normal


def make_frame(n):
    """mju_makeFrame as the kernels state it: the two tangents of a unit normal."""
    t1 = np.array([0.0, 1.0, 0.0]) if -0.5 < n[1] < 0.5 else np.array([0.0, 0.0, 1.0])
    t1 = t1 - (n @ t1) * n
    t1 /= np.linalg.norm(t1)
    return t1, np.cross(n, t1)


def expected_frame(m, n, g1, g2, geom_xmat):
    """The contact frame the row stage builds on normal n for the pair (g1, g2): mju_makeFrame, and for a plane - capsule pair (MuJoCo's frame
    for that pair type) the first tangent along the capsule's axis -- the third column of its geom_xmat -- made orthogonal to the normal,
    unless the axis is within 30 degrees of the normal."""
    t1, t2 = make_frame(n)
    if int(m.geom_type[g1]) == 0 and int(m.geom_type[g2]) == 3:
        ax = geom_xmat[g2][:, 2]
        y = ax - (ax @ n) * n
        if np.linalg.norm(y) >= 0.5:
            t1 = y / np.linalg.norm(y)
            t2 = np.cross(n, t1)
    return np.array([n, t1, t2])


def frame_error(m, con, frames, geom_xmat):
    """Largest entry by which the frames [n, 3, 3] of contacts `con` differ from expected_frame on their own normals."""
    return max((np.abs(F - expected_frame(m, c[4:7], int(c[7]), int(c[8]), geom_xmat)).max() for c, F in zip(con, frames)), default=0.0)


def bounds_from(worst):
    return np.maximum(4 * np.asarray(worst), FLOORS)


def f32_reference(m, qpos, hfields=None):
    """The float64 and float32 oracles over the same states: per state the float64 forward record, whether the float32 oracle has the same
    pair multiset, and the bounds = 4 x the largest float32 deviation (dist, pos, normal) over the agreeing states, floored."""
    from oracle.oracle import Oracle
    o64, o32 = Oracle(m.blob()), Oracle(m.blob(), f32=True)
    ref, agree, worst = [], [], np.zeros(3)
    for e, q in enumerate(qpos):
        hf = None if hfields is None else hfields[e]
        r64, r32 = oracle_forward(o64, m, q, hf), oracle_forward(o32, m, q, hf)
        same = pair_multiset(r64["contacts"]) == pair_multiset(r32["contacts"])
        if same:
            worst = np.maximum(worst, deviation(r64["contacts"], r32["contacts"]))
        ref.append(r64)
        agree.append(same)
    return ref, np.array(agree), np.maximum(4 * worst, FLOORS)


def link_frames(m, ref):
    """World frame of every link from the oracle's body frames: a link's frame is that of its first body (the one its joints belong to)."""
    bl = np.asarray(m.hip_body_link)
    pos, mat = [], []
    for l in range(int(bl.max()) + 1):
        b = int(np.flatnonzero(bl == l)[0])
        pos.append(ref["xpos"][b]); mat.append(ref["xmat"][b])
    return np.array(pos).reshape(-1, 3), np.array(mat).reshape(-1, 3, 3)


def compose(table, lpos, lmat, origin):
    """World positions [n, 3], rotations [n, 3, 3] and the extra point [n, 3] (bodies: the COM) of a host export table [n, 16] on given
    link frames (world-welded items: constant, relative to `origin`)."""
    x, R, a = [], [], []
    for r in table:
        l = int(r[0])
        p, Rl, ex = r[1:4], r[4:13].reshape(3, 3), r[13:16]
        if l < 0:
            x.append(p + origin); R.append(Rl); a.append(ex + origin)
        else:
            x.append(lpos[l] + lmat[l] @ p); R.append(lmat[l] @ Rl); a.append(lpos[l] + lmat[l] @ ex)
    return np.array(x).reshape(-1, 3), np.array(R).reshape(-1, 3, 3), np.array(a).reshape(-1, 3)


# ---- state families: {name: (qpos [N, nq] float32, hfields [N, nrow, ncol] or None)} per asset, N = 32 unless the family has fewer
N = 32


def _range_states(m, rng, n, frac):
    """Hinge / slide joints uniform in the inner `frac` of their range; everything else at qpos0."""
    lo, hi = np.asarray(m.jnt_range)[:, 0], np.asarray(m.jnt_range)[:, 1]
    q = np.tile(np.asarray(m.qpos0, float), (n, 1))
    for j in range(m.njnt):
        if int(m.jnt_type[j]) in (2, 3) and hi[j] > lo[j]:
            a = int(m.jnt_qposadr[j])
            mid, half = 0.5 * (lo[j] + hi[j]), 0.5 * (hi[j] - lo[j])
            q[:, a] = mid + frac * half * rng.uniform(-1, 1, n)
    return q


def _contact_free(m, rng, n):
    """States of the open hand that the float64 oracle finds free of contacts (rejection sampling around qpos0)."""
    from oracle.oracle import Oracle
    o = Oracle(m.blob())
    out = []
    lo, hi = np.asarray(m.jnt_range)[:, 0], np.asarray(m.jnt_range)[:, 1]
    for _ in range(40 * n):
        q = np.clip(np.asarray(m.qpos0, float) + rng.normal(0, 0.05, m.nq), lo, hi).astype(np.float32).astype(float)
        if len(oracle_forward(o, m, q)["contacts"]) == 0:
            out.append(q)
            if len(out) == n:
                break
    return np.array(out).reshape(-1, m.nq)


def _leg_states(m, rng, n, dz):
    """The walk keyframe with joint noise, the root moved by U(dz) in height and U(-0.5, 0.5) in x and y: tests/test_gpu_terrain.py's recipe
    (dz = +- 3 cm, on its height fields of up to 15 cm).  On the plane of myolegs the feet hover at the keyframe's own height and the root
    goes 3 to 8 cm lower.  (That lower root on the height fields puts the feet up to 7 cm INTO the terrain, where MPR reports contacts with
    the side walls of the prisms; such states are not what a step ever sees and are not used.)"""
    kq = np.asarray(m.key_qpos).reshape(-1, m.nq)[2]
    q = np.tile(kq, (n, 1))
    q[:, 7:] += rng.normal(0, 0.05, (n, m.nq - 7))
    q[:, 2] += rng.uniform(dz[0], dz[1], n)
    q[:, :2] += rng.uniform(-0.5, 0.5, (n, 2))
    return q


def _rollout_states(m, n, every=4, ctrl=0.0):
    """n states of one float64 oracle rollout from qpos0 under a constant control, one every `every` substeps."""
    from oracle.oracle import Oracle
    o = Oracle(m.blob())
    o.reset()
    o.set_state(ctrl=np.full(m.nu, ctrl))
    out = []
    for _ in range(n):
        assert o.step(every) == 0
        out.append(o.field("qpos").copy())
    return np.array(out)


def families(stem, m):
    rng = np.random.default_rng(sum(map(ord, stem)))
    f32 = np.float32
    if stem == "myohand_pose":
        return {"range90": (_range_states(m, rng, N, 0.9).astype(f32), None), "free": (_contact_free(m, rng, N).astype(f32), None)}
    if stem == "myohand_hold":
        import test_gpu_hold as TH
        return {"object_in_palm": (TH._states(m, N, 3)[0], None)}
    if stem == "myolegs":
        return {"feet_on_ground": (_leg_states(m, rng, N, (-0.08, -0.03)).astype(f32), None)}
    if stem == "myolegs_terrain":
        import test_gpu_terrain as TT
        return {"terrain": (_leg_states(m, rng, N, (-0.03, 0.03)).astype(f32), TT._grids(N, rng).astype(f32))}
    if stem == "myohand_baoding":
        import test_gpu_baoding as TB
        return {k: (TB._states(m, k, N, s)[0], None) for k, s in (("palm", 1), ("ballball", 2), ("pedestal", 3), ("floor", 4))}
    if stem == "myohand_die":
        import die_states as DS
        # die_states.py's episodes reach 20 contacts at most (none above NC = 32, let alone 64).  The crowded family: random hand poses over
        # 95 % of the joint ranges, the 16 of 200 with the most contacts in the float64 oracle (fingers crossing each other: up to 40)
        from oracle.oracle import Oracle
        o = Oracle(m.blob())
        Q = _range_states(m, rng, 200, 0.95).astype(f32)
        nc = np.array([len(oracle_forward(o, m, q.astype(float))["contacts"]) for q in Q])
        return {"rollout": (np.array([s[0] for s in DS.pick_states(DS.rollout_states(m), N)]).astype(f32), None), "crowded": (Q[np.argsort(-nc)[:16]], None)}
    if stem == "myohand_object_cup":
        return {"grasp": (cup_grasp_states(m), None)}
    if stem == "myohand_object_airplane":
        return {"rollout": (_rollout_states(m, N, every=8, ctrl=0.5).astype(f32), None)}      # the hand closes on the airplane lying on the table
    raise KeyError(stem)


ASSETS = ("myohand_pose", "myohand_hold", "myolegs", "myolegs_terrain", "myohand_baoding", "myohand_die", "myohand_object_airplane", "myohand_object_cup")


def cup_grasp_states(m):
    """Grasp frames of the reference's MyoHand_cup_drink1 motion on the cup asset (tests/test_gpu_track.py's recipe): a finger touches several
    of the cup's convex parts at once, and the deepest frames carry more than 64 contacts -- the second contact bank of the TRK class."""
    import os
    from myosuite_mjx_amd import track as T
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_motion.npz"))
    motion = {k.split("__in__")[1]: f[k] for k in f.files if k.startswith("track_MyoHand_cup_drink1__in__")}
    R, O = motion["robot"], motion["object"]
    rng = np.random.default_rng(3)
    frames = list(range(0, len(R), max(1, len(R) // 32)))[:32]
    q = np.zeros((len(frames), m.nq))
    for i, t in enumerate(frames):
        q[i, :29] = R[t] + rng.normal(0, 0.01, 29) * (np.arange(29) >= 6)
        q[i, 29:32] = O[t, :3]
        q[i, 32:35] = T.quat2euler(O[t, 3:])
    return q.astype(np.float32)
