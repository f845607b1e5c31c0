"""Host side of the forward pass (no GPU): the export tables myo_model_load builds from the blob, and the ids of the C header.

The kernel exports a body, site or geom as `link frame x (position, rotation inside the link)`.  Here the tables the library builds
(myo_forward_host_tables, float64) are composed in numpy with the ORACLE's link frames and compared with the oracle's own xpos / xmat /
xipos / geom_xpos / geom_xmat / site_xpos, for every committed asset the HIP path takes: a wrong link, a wrong composition order or a
world-welded item in the wrong coordinates shows up without a GPU."""
import glob
import os
import re

import numpy as np
import pytest

import forward_ref as FR
from myosuite_mjx_amd import capi
from myosuite_mjx_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stems():
    return sorted({re.sub(r"\.myob(\.gz)?$", "", os.path.basename(p)) for d in (M.ASSET_DIR, M.GOLDEN_DIR) for p in glob.glob(os.path.join(d, "*.myob*"))})


def _pose(m, rng):
    """qpos0 with every hinge / slide joint moved inside its range (free joints and their quaternions stay)."""
    q = np.array(m.qpos0, float)
    for j in range(m.njnt):
        if int(m.jnt_type[j]) in (2, 3):
            a = int(m.jnt_qposadr[j])
            lo, hi = m.jnt_range[j]
            q[a] = rng.uniform(lo, hi) if hi > lo else q[a] + rng.uniform(-0.3, 0.3)
    return q


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(capi.LIB_PATH):
        capi.build_library()


def test_tables_reproduce_the_oracle_frames_on_every_asset():
    from oracle.oracle import Oracle
    rng = np.random.default_rng(0)
    stems = _stems()
    assert len(stems) >= 61
    checked = 0
    for stem in stems:
        m = M.load_asset(stem)
        if "hip_unsupported" in m.arrays:
            continue
        body, site, geom = capi.forward_host_tables(m.blob())
        assert body.shape == (m.nbody, 16) and site.shape == (m.nsite, 16) and geom.shape == (m.ngeom, 16), stem
        assert np.array_equal(body[:, 0], np.asarray(m.hip_body_link, float)), stem
        assert np.array_equal(site[:, 13], np.asarray(m.site_bodyid, float)) and np.array_equal(geom[:, 13], np.asarray(m.geom_bodyid, float)), stem
        ref = FR.oracle_forward(Oracle(m.blob()), m, _pose(m, rng))
        lpos, lmat = FR.link_frames(m, ref)
        org = np.asarray(m.hip_origin, float)
        # (link frames from the oracle are world coordinates: the moving items need no origin; the static ones are stored relative to it)
        x, R, com = FR.compose(body, lpos, lmat, org)
        assert np.abs(x - ref["xpos"]).max() < 1e-12 and np.abs(R - ref["xmat"]).max() < 1e-12 and np.abs(com - ref["xipos"]).max() < 1e-12, stem
        x, R, _ = FR.compose(geom, lpos, lmat, org)
        assert np.abs(x - ref["geom_xpos"]).max() < 1e-12 and np.abs(R - ref["geom_xmat"]).max() < 1e-12, stem
        x, R, _ = FR.compose(site, lpos, lmat, org)
        assert np.abs(x - ref["site_xpos"]).max() < 1e-12, stem
        if ref["site_xmat"] is not None:
            assert np.abs(R - ref["site_xmat"]).max() < 1e-12, stem
        checked += 1
    assert checked >= 55, checked


def test_tables_refuse_a_blob_that_is_not_one():
    with pytest.raises(capi.MyoError):
        capi.forward_host_tables(b"NOPE" + bytes(60))


def test_ids_and_constants_equal_the_header():
    hdr = open(os.path.join(ROOT, "include", "myo_hip_forward.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    enums = {n: int(v) for n, v in re.findall(r"\b(MYO_FWD_[A-Z_]+)\s*=\s*(\d+)", body)}
    names = ("XPOS", "XMAT", "XIPOS", "SITE_XPOS", "SITE_XMAT", "GEOM_XPOS", "GEOM_XMAT", "NCON", "CONTACT", "COUNT")
    assert sorted(enums) == sorted("MYO_FWD_" + n for n in names)
    for n in names:
        assert getattr(capi, "FWD_" + n) == enums["MYO_FWD_" + n], n
    assert sorted(capi.FWD_NAMES.values()) == list(range(capi.FWD_COUNT))
    assert int(re.search(r"#define\s+MYO_FWD_CONTACT_WORDS\s+(\d+)", body).group(1)) == capi.FWD_CONTACT_WORDS == 16
    # the extension header is not part of myo_hip.h (whose declarations the oracle's ABI twin must all export)
    assert "myo_hip_forward.h" not in open(os.path.join(ROOT, "include", "myo_hip.h")).read()
    for fn in ("myo_forward", "myo_forward_buffer", "myo_forward_read", "myo_model_forward_dims", "myo_forward_host_tables"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, body), fn
        getattr(capi.lib(), fn)


def test_header_is_plain_c(tmp_path):
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "include/myo_hip_forward.h"\nint main(void) { return MYO_FWD_COUNT == 9 && MYO_FWD_CONTACT_WORDS == 16 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", ROOT, "-c", str(src), "-o", str(tmp_path / "a.o")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", ROOT, "-x", "c++", "-c", str(src), "-o", str(tmp_path / "b.o")])
