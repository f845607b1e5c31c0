"""Pen states for the plane - cylinder narrow phase (mjc_PlaneCylinder): the pen over the scene's floor, off the pedestal, in the four
branches.  The float64 oracle filters a cylinder pair by the distance of the other geom's centre along the cylinder axis, so the pen stands
at (0, 1.5, z): its axis, in the x-z plane, stays across the floor's centre.  Shared by tests/test_pen_host.py and tests/test_gpu_pen.py."""
import numpy as np

FLOOR_Z = -0.4
R, HH = 0.015, 0.065


def floor_qpos(m, phi, dist0):
    """qpos of the fully open hand with the pen's centre at (0, 1.5, FLOOR_Z + dist0) and its axis tilted by phi from the vertical in the
    x-z plane (the Object body's compiled frame is a rotation about y, so the pen's y hinge sets the tilt)."""
    ob = m.name2id("body", "Object")
    q0 = np.asarray(m.body_quat[ob], float)
    th0 = 2 * np.arctan2(q0[2], q0[0])
    q = np.zeros(m.nq)
    c, s = np.cos(th0), np.sin(th0)
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])     # the slides move along the body's compiled frame
    q[-6:-3] = Ry.T @ (np.array([0.0, 1.5, FLOOR_Z + dist0]) - np.asarray(m.body_pos[ob], float))
    q[-2] = phi - th0
    return q


def branch_states(m):
    """(name, qpos, expected number of pen - floor contacts) for 1, 2, 3 and 4 contacts (margins are 0: four contacts need a pen sunk
    below half its radius)."""
    out = []
    phi = 0.5
    out.append(("rim", floor_qpos(m, phi, HH * np.cos(phi) + R * np.sin(phi) - 0.002), 1))
    out.append(("side", floor_qpos(m, np.pi / 2 - 1e-3, R - 0.002), 2))
    phi = 0.02
    out.append(("cap", floor_qpos(m, phi, HH * np.cos(phi) + R * np.sin(phi) - 0.002), 3))
    out.append(("sunk", floor_qpos(m, np.pi / 2 - 1e-3, -0.6 * R), 4))
    return out
