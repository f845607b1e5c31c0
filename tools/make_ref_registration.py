"""Numbers of the reference's registration files that the CPU tests check the port's tables against, stored as data under tests/golden/
so that the suite runs from a clean checkout alone (parsed as text; nothing is imported or executed).  Run where the reference tree is
present; the output is committed:
  tests/golden/ref_registration.json     envs/myo/myobase/__init__.py: the ASL_qpos rows and the myoHandPoseFixed-v0 target;
                                         envs/myo/myodm/__init__.py: the OBJECTS tuple and the MyoHand task_spec entries

    python tools/make_ref_registration.py"""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MYO_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")


def registration():
    txt = open(os.path.join(REF, "myosuite/envs/myo/myobase/__init__.py")).read()
    rows = re.findall(r'ASL_qpos\[(\d)\] = \(\s*"([^"]+)"', txt)
    assert len(rows) == 10
    asl = {k: [float(x) for x in s.split(" ")] for k, s in rows}
    blk = txt[txt.index('id="myoHandPoseFixed-v0"'):]
    blk = blk[blk.index("np.array("):blk.index("),", blk.index("np.array("))]
    pose = [float(x) for x in re.findall(r"-?\d+\.?\d*(?:e-?\d+)?", blk.replace("np.array(", ""))]
    src = open(os.path.join(REF, "myosuite/envs/myo/myodm/__init__.py")).read()
    tasks = re.findall(r'task_spec\(\s*name="([^"]+)",\s*robot="MyoHand",\s*object="([^"]+)",\s*motion="([^"]+)"', src)
    objects = re.findall(r'"([^"]+)"', re.search(r'OBJECTS = \((.*?)\)', src, re.S).group(1))
    json.dump({"myobase": {"ASL_qpos": asl, "myoHandPoseFixed-v0_target": pose},
               "myodm": {"objects": objects, "tasks": [list(t) for t in tasks]}},
              open(os.path.join(OUT, "ref_registration.json"), "w"), indent=0)


if __name__ == "__main__":
    registration()
