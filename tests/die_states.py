"""States of the die task taken from oracle rollouts, shared by tests/test_die_host.py and tests/test_gpu_die.py: episodes of the env's own
loop (muscle sigmoid, 5 substeps per env step) from the task's reset pose, one with zero actions and three with U(-1, 1) actions.  Every
recorded state carries what the die touches: "palm" (a metacarpal or carpal body), "finger" (a phalanx), "falling" (no die contact, moving
down), and the geom-type pairs of its contacts (3 = capsule, 6 = box)."""
import numpy as np

FRAME_SKIP = 5
PHALANX = ("proxph", "midph", "distph", "proximal_thumb", "distal_thumb")


def init_qpos(m):
    q = np.array(m.qpos0, float)
    q[:-7] = 0.0
    q[0] = -1.5
    return q


def muscle_ctrl(a):
    return 1.0 / (1.0 + np.exp(-5.0 * (np.asarray(a, float) - 0.5)))      # base_v0.py:87-91


def die_geoms(m):
    ob = m.name2id("body", "Object")
    return [g for g in range(m.ngeom) if m.geom_bodyid[g] == ob]


def tag_state(m, o, dg):
    """Tags of the oracle's current (forwarded) state and the geom-type pairs of the die's contacts."""
    pairs = [(int(c[7]), int(c[8])) for c in o.contacts() if int(c[7]) in dg or int(c[8]) in dg]
    bodies = {m.names["body"][m.geom_bodyid[g]] for p in pairs for g in p if g not in dg}
    types = {tuple(sorted((int(m.geom_type[a]), int(m.geom_type[b])))) for a, b in pairs}
    tags = set()
    if any(n.startswith(PHALANX) for n in bodies):
        tags.add("finger")
    if any(not n.startswith(PHALANX) for n in bodies):
        tags.add("palm")
    if not pairs and o.field("qvel")[-4] < -0.2:
        tags.add("falling")
    return tags, types


def rollout_states(m, steps=150, seeds=(None, 1, 2, 3)):
    """[(qpos, qvel, act, tags, types, ncon, nefc, iters)] of every env step of the four episodes (the state after the step, forwarded)."""
    from oracle.oracle import Oracle
    o = Oracle(m.blob())
    dg = die_geoms(m)
    out = []
    for seed in seeds:
        rng = np.random.default_rng(0 if seed is None else seed)
        o.reset()
        o.set_state(qpos=init_qpos(m))
        for _ in range(steps):
            a = np.zeros(m.nu) if seed is None else rng.uniform(-1, 1, m.nu)
            o.set_state(ctrl=muscle_ctrl(a))
            ncon = nefc = it = 0
            for _ in range(FRAME_SKIP):
                assert o.step(1) == 0
                ncon, nefc, it = max(ncon, o.ncon), max(nefc, o.nefc), max(it, o.solver_iter)
            o.forward()
            tags, types = tag_state(m, o, dg)
            out.append((o.field("qpos").copy(), o.field("qvel").copy(), o.field("act").copy(), tags, types, ncon, nefc, it))
    return out


def pick_states(states, n=48):
    """n states for a one-step comparison: the three kinds in turn (resting on the palm = palm contact at low die speed), states with
    capsule - box contacts first within a kind; the die still inside its slide range (a state at the range's end adds a joint-limit impact)."""
    ok = [s for s in states if np.abs(s[0][-6:-3]).max() < 0.22]
    kinds = {
        "palm": [s for s in ok if "palm" in s[3] and np.abs(s[1][-6:-3]).max() < 0.5],
        "finger": [s for s in ok if "finger" in s[3]],
        "falling": [s for s in ok if "falling" in s[3]],
    }
    for k in kinds:
        kinds[k].sort(key=lambda s: (3, 6) not in s[4])
    picked, i = [], 0
    while len(picked) < n and any(kinds.values()):
        for k in ("palm", "finger", "falling"):
            if kinds[k] and len(picked) < n:
                s = kinds[k].pop(0)
                if not any(s is p for p in picked):
                    picked.append(s)
        i += 1
    return picked
