"""Goal-trajectory fixture of the baoding task: tests/golden/baoding_goal_traj.npz.

Runs the reference's BaodingEnvV1.create_goal_trajectory (envs/myo/myochallenge/baoding_v1.py) for the three directions and a few
(time step, period) pairs.  The reference's env module needs MuJoCo to import, so only the Task enum and that one method are taken from its
source and run on a stub.  Runs where the reference tree is present; usage: python tools/make_baoding_goal_fixture.py"""
import ast
import enum
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MYO_REFERENCE", "/root/reference")
SRC = os.path.join(REF, "myosuite", "envs", "myo", "myochallenge", "baoding_v1.py")


def reference_functions():
    tree = ast.parse(open(SRC).read())
    task = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Task")
    env = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "BaodingEnvV1")
    fn = next(n for n in env.body if isinstance(n, ast.FunctionDef) and n.name == "create_goal_trajectory")
    ns = {"np": np, "enum": enum}
    exec(compile(ast.Module(body=[task, fn], type_ignores=[]), SRC, "exec"), ns)
    return ns["Task"], ns["create_goal_trajectory"]


if __name__ == "__main__":
    Task, create = reference_functions()
    cases = [(sign, dt, period) for sign in (0, -1, 1) for dt, period in ((0.025, 5.0), (0.025, 4.0), (0.025, 6.0), (0.1, 6.0))]
    which = {0: Task.HOLD, -1: Task.BAODING_CW, 1: Task.BAODING_CCW}
    trajs = []
    for sign, dt, period in cases:
        stub = type("Stub", (), {"which_task": which[sign]})()
        trajs.append(create(stub, time_step=dt, time_period=period))
    out = os.path.join(ROOT, "tests", "golden", "baoding_goal_traj.npz")
    np.savez_compressed(out, cases=np.array(cases, np.float64), goal=np.array(trajs, np.float64))
    print(out, np.array(trajs).shape)
