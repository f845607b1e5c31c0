"""Compiled-model container: arrays (mjModel naming) + names, (de)serialised as a
MYOB blob (`blob.py`) plus a JSON name side-car.

The MJCF sources live in the reference tree, which does not exist on the GPU box, so the
compiled blobs for the config models are committed under `myosuite_mjx_amd/assets/`
(data, produced by `tools/compile_models.py` from the reference's model files)."""
from __future__ import annotations

import json
import os

import numpy as np

from . import blob as _blob

ASSET_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")
# compiled models added since the seed assets are data fixtures of the repository (tests/golden/, like every other binary derived from the
# reference's files); load_asset looks there after ASSET_DIR
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


class Model:
    def __init__(self, arrays: dict, names: dict, source: str = ""):
        self.arrays = arrays
        self.names = names
        self.source = source
        self._blob = None

    def __getattr__(self, k):
        arrays = self.__dict__.get("arrays", {})
        if k in arrays:
            return arrays[k]
        raise AttributeError(k)

    # sizes, mjModel style
    @property
    def nq(self): return int(self.arrays["sizes"][0])
    @property
    def nv(self): return int(self.arrays["sizes"][1])
    @property
    def nu(self): return int(self.arrays["sizes"][2])
    @property
    def na(self): return int(self.arrays["sizes"][3])     # activation slots of the state arrays (one per actuator)

    @property
    def n_muscle(self):
        """MuJoCo's na for these models: actuators with an activation state (muscles); stateless motors keep an unused slot."""
        return int((np.asarray(self.arrays["actuator_kind"]) == 0).sum())
    @property
    def nbody(self): return int(self.arrays["sizes"][4])
    @property
    def njnt(self): return int(self.arrays["sizes"][5])
    @property
    def ngeom(self): return int(self.arrays["sizes"][6])
    @property
    def nsite(self): return int(self.arrays["sizes"][7])
    @property
    def ntendon(self): return int(self.arrays["sizes"][8])
    @property
    def timestep(self): return float(self.arrays["opt"][0])

    def name2id(self, kind, name):
        return self.names[kind].index(name)

    # mujoco_py-style accessors the reference patches onto MjModel (physics/mj_sim_scene.py:110-163)
    def _n2i(self, kind, name):
        if kind not in self.names or name not in self.names[kind]:
            raise ValueError('No {} with name "{}" exists.'.format(kind, name))
        return self.names[kind].index(name)

    def body_name2id(self, name): return self._n2i("body", name)
    def geom_name2id(self, name): return self._n2i("geom", name)
    def site_name2id(self, name): return self._n2i("site", name)
    def joint_name2id(self, name): return self._n2i("joint", name)
    def actuator_name2id(self, name): return self._n2i("actuator", name)
    def tendon_name2id(self, name): return self._n2i("tendon", name)
    def camera_name2id(self, name): return self._n2i("camera", name)      # (cameras / sensors are not compiled: always "No camera ...")
    def sensor_name2id(self, name): return self._n2i("sensor", name)

    def blob(self) -> bytes:
        if self._blob is None:
            self._blob = _blob.pack(self.arrays)
        return self._blob

    def with_sarcopenia(self) -> "Model":
        """Copy of the model with the muscle condition "sarcopenia" applied (BaseV0.initializeConditions,
        envs/myo/base_v0.py:64-68): the peak force entry of every actuator's gainprm is halved (biasprm is left alone)."""
        arrays = {k: np.array(v, copy=True) for k, v in self.arrays.items()}
        gp = arrays["actuator_gainprm"].reshape(self.nu, -1)
        gp[:, 2] *= 0.5
        if "hip_act" in arrays:
            act = arrays["hip_act"].reshape(self.nu, -1)
            pos = gp[:, 2] >= 0          # a negative entry means "scale / acc0", which the halving does not change
            act[pos, 2] = gp[pos, 2]
        return Model(arrays, self.names, self.source)

    def with_body_mass(self, body, mass) -> "Model":
        """Copy of the model with `body_mass[body] = mass` for every env (`body`: id or name), as `model.body_mass[bid] = ...` edits a
        compiled MuJoCo model (PoseEnvV0.reset, envs/myo/myobase/pose_v0.py:163-176).  The mass, COM and inertia about the COM of the
        body's link (the bodies welded together, lowering.py) are recomposed in float64 with lowering's formulas; nothing else changes
        (body_inertia, acc0, invweights and lengthranges keep their values, as without mj_setConst)."""
        from .lowering import _rel_transforms
        from .mjcf import quat2mat
        b = self.body_name2id(body) if isinstance(body, str) else int(body)
        if not 0 <= b < self.nbody:
            raise ValueError(f"no body {body!r}")
        if not mass >= 0:
            raise ValueError("body mass must be >= 0")
        arrays = {k: np.array(v, copy=True) for k, v in self.arrays.items()}
        arrays["body_mass"][b] = float(mass)
        out = Model(arrays, self.names, self.source)
        link = int(arrays["hip_body_link"][b]) if "hip_body_link" in arrays else -1
        if link < 0:                     # welded to the world (or no HIP tables): no link to recompose
            return out
        _, Rrel, prel = _rel_transforms(out)
        members = [k for k in range(1, self.nbody) if int(arrays["hip_body_link"][k]) == link]
        bm, ipos, iquat, inertia = arrays["body_mass"], arrays["body_ipos"], arrays["body_iquat"], arrays["body_inertia"]
        tot = sum(bm[k] for k in members)
        com = sum(bm[k] * (prel[k] + Rrel[k] @ ipos[k]) for k in members) / tot
        I = np.zeros((3, 3))
        for k in members:
            Ri = Rrel[k] @ quat2mat(iquat[k])
            d = prel[k] + Rrel[k] @ ipos[k] - com
            I += Ri @ np.diag(inertia[k]) @ Ri.T + bm[k] * (d @ d * np.eye(3) - np.outer(d, d))
        lm, lc, li = arrays["hip_link_mass"], arrays["hip_link_com"], arrays["hip_link_inertia"]
        lm.reshape(-1)[link] = tot
        lc.reshape(-1, 3)[link] = com
        li.reshape(-1, 6)[link] = [I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]
        return out

    def with_geom_params(self, geoms, size=None, pos=None, friction=None) -> "Model":
        """Copy of the model with `geom_size[geoms]`, `geom_pos[geoms]` and / or `geom_friction[geoms]` set for every env (`geoms`: ids or
        names; each array [len(geoms), 3], None: unchanged), as BaodingEnvV1.reset and ReorientEnvV0.reset edit a compiled MuJoCo model
        (baoding_v1.py:360-385, reorient_v0.py:221-247).  geom_rbound follows the new size as the compiler would set it; the HIP tables
        are lowered again from the edited arrays.  Nothing else changes (masses, inertias, invweights keep their values, as without
        mj_setConst).  Primitive geoms only (a mesh's shape is its vertex table)."""
        from .lowering import lower
        from .mjcf import GEOM_BOX, GEOM_CAPSULE, GEOM_CYLINDER, GEOM_ELLIPSOID, GEOM_SPHERE, CompiledModel, geom_rbound
        ids = [self.geom_name2id(g) if isinstance(g, str) else int(g) for g in geoms]
        for g in ids:
            if not 0 <= g < self.ngeom:
                raise ValueError(f"no geom {g!r}")
        arrays = {k: np.array(v, copy=True) for k, v in self.arrays.items()}
        for name, val, nonneg in (("geom_size", size, True), ("geom_pos", pos, False), ("geom_friction", friction, True)):
            if val is None:
                continue
            val = np.asarray(val, float).reshape(len(ids), 3)
            if not np.isfinite(val).all() or (nonneg and (val < 0).any()):
                raise ValueError(f"{name} must be finite" + (" and >= 0" if nonneg else ""))
            arrays[name][ids] = val
        for g in ids:
            if int(arrays["geom_type"][g]) not in (GEOM_SPHERE, GEOM_CAPSULE, GEOM_ELLIPSOID, GEOM_CYLINDER, GEOM_BOX):
                raise NotImplementedError("with_geom_params: sphere / capsule / ellipsoid / cylinder / box geoms only")
            arrays["geom_rbound"][g] = geom_rbound(int(arrays["geom_type"][g]), arrays["geom_size"][g])
        if "hip_cg_link" in arrays:
            cm = CompiledModel(arrays={k: v for k, v in arrays.items() if not k.startswith("hip_")}, names=self.names)
            lower(cm)
            arrays = cm.arrays
        return Model(arrays, self.names, self.source)

    def with_body_pos(self, body, pos) -> "Model":
        """Copy of the model with `body_pos[body] = pos` (`body`: id or name), as KeyTurnEnvV0.reset moves the key
        (envs/myo/myobase/key_turn_v0.py:164-167).  The HIP tables follow for a body that heads a kinematic root link (its link origin moves
        by the same amount), and for a jointless child of the world (ReorientEnvV0.reset moves the die's target,
        envs/myo/myochallenge/reorient_v0.py:210-215: its static geoms and sites are lowered again); nothing else changes (inertias,
        invweights and lengthranges keep their values, as without mj_setConst)."""
        b = self.body_name2id(body) if isinstance(body, str) else int(body)
        if not 0 < b < self.nbody:
            raise ValueError(f"no movable body {body!r}")
        pos = np.asarray(pos, float).reshape(3)
        if not np.isfinite(pos).all():
            raise ValueError("body position must be finite")
        arrays = {k: np.array(v, copy=True) for k, v in self.arrays.items()}
        delta = pos - arrays["body_pos"][b]
        arrays["body_pos"][b] = pos
        if "hip_body_link" in arrays and int(arrays["body_jntnum"][b]) == 0 and int(arrays["body_parentid"][b]) == 0:
            # a jointless child of the world (myohand_die's target, ReorientEnvV0.reset): static geoms and sites, lowered again
            from .lowering import lower
            from .mjcf import CompiledModel
            cm = CompiledModel(arrays={k: v for k, v in arrays.items() if not k.startswith("hip_")}, names=self.names)
            lower(cm)
            arrays = cm.arrays
        elif "hip_body_link" in arrays:
            link = int(arrays["hip_body_link"][b])
            heads = link >= 0 and int(arrays["hip_link_parent"][link]) < 0 and int(arrays["body_parentid"][b]) == 0 and \
                min(k for k in range(1, self.nbody) if int(arrays["hip_body_link"][k]) == link) == b
            if not heads:
                raise NotImplementedError("with_body_pos: only a child of the world heading a root link (the HIP tables would need re-lowering)")
            arrays["hip_link_pos"].reshape(-1, 3)[link] += delta
        return Model(arrays, self.names, self.source)

    def with_body_quat(self, body, quat) -> "Model":
        """Copy of the model with `body_quat[body] = quat` (`body`: id or name), as PenTwirlRandomEnvV0.reset turns the target
        (envs/myo/myobase/pen_v0.py:173-184).  World-welded bodies only (no joints, the world as parent): their geoms and sites are static,
        and the HIP tables are lowered again from the edited arrays."""
        from .lowering import lower
        from .mjcf import CompiledModel
        b = self.body_name2id(body) if isinstance(body, str) else int(body)
        if not 0 < b < self.nbody:
            raise ValueError(f"no movable body {body!r}")
        if int(self.arrays["body_jntnum"][b]) != 0 or int(self.arrays["body_parentid"][b]) != 0:
            raise NotImplementedError("with_body_quat: only a jointless child of the world")
        quat = np.asarray(quat, float).reshape(4)
        if not np.isfinite(quat).all() or abs(np.linalg.norm(quat) - 1) > 1e-6:
            raise ValueError("body quaternion must be a finite unit quaternion")
        arrays = {k: np.array(v, copy=True) for k, v in self.arrays.items()}
        arrays["body_quat"][b] = quat
        if "hip_cg_link" in arrays:
            cm = CompiledModel(arrays={k: v for k, v in arrays.items() if not k.startswith("hip_")}, names=self.names)
            lower(cm)
            arrays = cm.arrays
        return Model(arrays, self.names, self.source)

    def with_integrator(self, name) -> "Model":
        """Copy of the model with `<option integrator=...>` set: "Euler" (semi-implicit, implicit joint damping) or "RK4" (mj_RungeKutta)."""
        if name not in ("Euler", "RK4"):
            raise ValueError("integrator must be 'Euler' or 'RK4'")
        arrays = {k: np.array(v, copy=True) for k, v in self.arrays.items()}
        arrays["integrator"] = np.array([1 if name == "RK4" else 0], np.int32)
        return Model(arrays, self.names, self.source)

    def save(self, stem, compress=False):
        """MYOB blob + JSON name side-car.  compress=True writes `<stem>.myob.gz` (the hull vertex graphs of the MyoDM objects shrink ~6x)."""
        if compress:
            import gzip
            with open(stem + ".myob.gz", "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0) as f:
                f.write(self.blob())
        else:
            with open(stem + ".myob", "wb") as f:
                f.write(self.blob())
        with open(stem + ".json", "w") as f:
            json.dump({"names": self.names, "source": os.path.basename(self.source)}, f)

    @classmethod
    def load(cls, stem):
        if os.path.exists(stem + ".myob"):
            with open(stem + ".myob", "rb") as f:
                b = f.read()
        else:
            import gzip
            with gzip.open(stem + ".myob.gz", "rb") as f:
                b = f.read()
        with open(stem + ".json") as f:
            meta = json.load(f)
        m = cls(_blob.unpack(b), meta["names"], meta.get("source", ""))
        m._blob = b
        return m


def from_mjcf(path, terrain=False, replace=None, convex_meshes=False) -> Model:
    """Compile an MJCF file (needs the reference tree; not available on the GPU box)."""
    from .mjcf import compile_mjcf
    from .setconst import set_constants
    from .lowering import lower
    cm = compile_mjcf(path, terrain, replace, convex_meshes)
    set_constants(cm)
    try:
        lower(cm)
    except NotImplementedError as e:     # model is oracle-only for now: myo_model_load will refuse it (no hip_* tables)
        cm.arrays["hip_unsupported"] = np.frombuffer(str(e).encode()[:200].ljust(4, b" "), dtype=np.uint8).astype(np.int32)
    return Model(cm.arrays, cm.names, path)


def asset_stem(name) -> str:
    """Path stem of a committed compiled model: under ASSET_DIR, else under GOLDEN_DIR (e.g. 'myohand_keyturn')."""
    for d in (ASSET_DIR, GOLDEN_DIR):
        stem = os.path.join(d, name)
        if os.path.exists(stem + ".myob") or os.path.exists(stem + ".myob.gz"):
            return stem
    raise FileNotFoundError(f"compiled model {name!r} not found under {ASSET_DIR} or {GOLDEN_DIR}; run tools/compile_models.py")


# arrays a model with touch sensors carries on top of the older ones (mjcf.py / lowering.py).  For the committed models they live in a
# side-car blob of their own, tests/golden/sensors/<name>.myob.gz (+ a JSON with the sensor names): the model's own blob stays what it was
SENSOR_ARRAYS = ("site_quat", "site_type", "site_size", "sensor_type", "sensor_objid", "sensor_adr", "hip_cg_body", "hip_touch")
SENSOR_DIR = os.path.join(GOLDEN_DIR, "sensors")


def split_sensor_arrays(m: Model):
    """(model without the sensor arrays, side-car Model holding only them or None): how tools/compile_models.py stores a compiled model."""
    if "hip_touch" not in m.arrays:
        return m, None
    base = Model({k: v for k, v in m.arrays.items() if k not in SENSOR_ARRAYS}, {k: v for k, v in m.names.items() if k != "sensor"}, m.source)
    side = Model({k: m.arrays[k] for k in SENSOR_ARRAYS}, {"sensor": list(m.names.get("sensor", []))}, m.source)
    return base, side


def load_asset(name) -> Model:
    """Load a committed compiled model by stem (e.g. 'myohand_pose'), with its sensor side-car merged in where it has one."""
    m = Model.load(asset_stem(name))
    side = os.path.join(SENSOR_DIR, name)
    if os.path.exists(side + ".myob.gz") and "hip_touch" not in m.arrays:
        s = Model.load(side)
        m = Model({**m.arrays, **s.arrays}, {**m.names, **s.names}, m.source)      # (the blob is packed again from the merged arrays)
    return m
