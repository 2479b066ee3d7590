"""Projective depth-image integration without a device: the numpy restatement (tests/projective_ref.py) against hand-worked
voxels, vgx_tsdf_projective_box (host only) against the restatement's box, the new symbols and their refusals, and that the
scenes of tests/test_projective_gpu.py reach every branch of the rules."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import projective_ref as P
from tests import projective_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ["vgx_tsdf_integrate_depth_image", "vgx_tsdf_integrate_depth_image_device", "vgx_tsdf_projective_box"]


@pytest.fixture(scope="module")
def capi():
    from voxgraph_amd import capi as m
    m.load()
    return m


def test_hand_worked_voxels_in_front_of_a_wall():
    """A fronto-parallel wall at z = 1 m (32FC1: d = 1 exactly), identity orientation, voxel 0.1 m, 8 voxels a side,
    truncation 0.3 m.  The camera centre sits at (0.05, 0.05, 0): on the axis of the voxel column (0, 0, vz), whose centres
    (0.05, 0.05, (vz + 0.5) 0.1) are then on the optical axis: x = y = 0, s = 1, r_v = z, sdf = 1 - z, weight 1 / 1^2 = 1."""
    img = P.Image(9, 7, P.DEPTH_32FC1, np.full((7, 9), 1.0, "<f4").view(np.uint8))
    cam = P.Camera(fx=6.0, fy=6.0, cx=4.0, cy=3.0)
    cfg = P.Config(default_truncation_distance=0.3, max_ray_length_m=5.0, min_ray_length_m=0.1)
    T = np.array([1, 0, 0, 0, F(0.5) * F(0.1), F(0.5) * F(0.1), 0], F)
    L = P.Layer(0.1, 8)
    fr = P.integrate(L, T, img, cam, cfg)
    column = {}
    for b, (bi, branch) in enumerate(zip(fr.voxel, fr.branch)):
        for k in np.nonzero((bi[:, 0] == 0) & (bi[:, 1] == 0))[0]:
            vz = int(bi[k, 2])
            slot = L.index.get((0, 0, vz // 8), -1)
            held = (L.distance[slot, vz % 8 * 64], L.weight[slot, vz % 8 * 64], L.rgba[slot, vz % 8 * 64]) if slot >= 0 else None
            column[vz] = (int(branch[k]), held)
    white = 0xffffffff
    # vz = 9: z = 0.95, sdf = 0.05 inside the band: the voxel becomes (sdf, 1, white)
    assert column[9] == (P.UPDATED, (F(1) - F(9.5) * F(0.1), F(1), white)) and abs(column[9][1][0] - 0.05) < 1e-6
    # vz = 10: z = 1.05, sdf = -0.05: behind the surface but not below -voxel_size: full weight
    assert column[10] == (P.UPDATED, (F(1) - F(10.5) * F(0.1), F(1), white)) and abs(column[10][1][0] + 0.05) < 1e-6
    # vz = 11: sdf = -0.15 < -0.1: the drop-off, w = 1 (0.3 - 0.15) / (0.3 - 0.1) = 0.75
    d, w, c = column[11][1]
    assert column[11][0] == P.UPDATED and abs(d + 0.15) < 1e-6 and abs(w - 0.75) < 1e-6 and c == white
    sdf = F(1) - F(11.5) * F(0.1)
    assert w == (F(1) * (F(0.3) + sdf)) / (F(0.3) - F(0.1)) and d == sdf
    # vz = 12: sdf = -0.25: w = 0.05 / 0.2 = 0.25
    assert column[12][0] == P.UPDATED and abs(column[12][1][1] - 0.25) < 1e-6 and abs(column[12][1][0] + 0.25) < 1e-6
    # vz = 13: sdf = -0.35 < -truncation: behind, untouched (its block exists: vz = 8 .. 12 are in it)
    assert column[13] == (P.BEHIND, (F(0), F(0), 0))
    # vz = 5: z = 0.55, sdf = 0.45 > truncation: carved -- the distance is clamped, the colour is NOT blended
    assert column[5] == (P.CARVED, (F(0.3), F(1), 0))
    # vz = 0: z = 0.05, r_s = 1 >= min_ray_length_m: carved too;  vz = -1: behind the camera, no pixel
    assert column[0] == (P.CARVED, (F(0.3), F(1), 0)) and column[-1][0] == P.NO_PIXEL
    assert fr.dropped_off.sum() > 0 and fr.counts["n_cleared"] == 0
    # a second frame: weights add, the distance is the weighted mean (here: the same), the carved voxel stays uncoloured
    P.integrate(L, T, img, cam, cfg)
    s0, s1 = L.index[(0, 0, 1)], L.index[(0, 0, 0)]
    assert L.weight[s0, 1 * 64] == F(2) and L.distance[s0, 1 * 64] == F(1) - F(9.5) * F(0.1) and L.rgba[s0, 1 * 64] == white
    assert L.weight[s1, 5 * 64] == F(2) and L.rgba[s1, 5 * 64] == 0
    # a wall beyond max_ray_length_m: a clearing pixel, sdf = max_ray_length_m - r_v wherever r_v + truncation <= max_ray_length_m
    far = P.Image(9, 7, P.DEPTH_32FC1, np.full((7, 9), 6.0, "<f4").view(np.uint8))
    L2 = P.Layer(0.1, 8)
    fr2 = P.integrate(L2, T, far, cam, cfg)
    on_axis = (fr2.voxel[..., 0] == 0) & (fr2.voxel[..., 1] == 0)
    vz = fr2.voxel[..., 2]
    assert (fr2.branch[on_axis & (vz >= 0) & (vz <= 46)] == P.CLEARED).all()            # z <= 4.65: 4.65 + 0.3 <= 5
    assert (fr2.branch[on_axis & (vz >= 47) & (vz <= 52)] == P.CLEAR_REFUSED).all()     # z >= 4.75
    assert fr2.counts["n_cleared"] == fr2.counts["n_updates"] > 0 and fr2.counts["n_carved"] == 0
    assert L2.distance[L2.index[(0, 0, 5)], 0] == F(0.3) and L2.weight[L2.index[(0, 0, 5)], 0] == F(1) / (F(6) * F(6))


def _poses():
    rng = np.random.default_rng(12)
    yaw = lambda a: S.quat([0, 0, 1], a)
    out = [S.IDENTITY, S.pose(yaw(np.pi / 2), [0.3, -0.2, 0.1]), S.pose(yaw(np.pi), [1.0, 2.0, -0.5]),
           S.pose(yaw(-np.pi / 2), [0, 0, 0]), S.TILTED, S.far_from_origin(S.TILTED),
           S.pose(S.quat([1, 0, 0], np.pi / 2), [-40 * 0.8 - 0.3, -40 * 0.8 - 0.1, -40 * 0.8 - 0.7]),
           S.pose(S.quat([0, 1, 0], np.pi), [-32.0, -32.0, -32.0])]
    for _ in range(6):
        q = rng.normal(size=4)
        out.append(S.pose(q / np.linalg.norm(q), rng.uniform(-60, 60, 3)))
    return out


def test_the_box_equals_the_restatement(capi):
    cfgs = [S.config(0.1), S.config(0.05, max_ray_length_m=2.5)]
    cams = [P.Camera(**S.CAMERA), P.Camera(fx=525.0, fy=525.0, cx=319.5, cy=239.5, max_depth_m=3.5),
            P.Camera(fx=-38.0, fy=37.0, cx=23.3, cy=15.6, min_depth_m=0.5, max_depth_m=8.0)]
    n = 0
    for T in _poses():
        for cfg in cfgs:
            for cam, (w, h) in zip(cams, ((48, 32), (640, 480), (48, 32))):
                for vs, vps in ((0.1, 8), (0.05, 16), (0.05, 8)):
                    lay = capi.depth_image_layout(width=w, height=h, encoding=capi.DEPTH_32FC1)
                    rc, lo, hi = capi.projective_box(lay, cam.capi(capi), cfg.capi(capi), T, vs, vps)
                    code, rlo, rhi = P.box(w, h, cam, cfg, T, vs, vps)
                    assert rc == code == capi.OK and np.array_equal(lo, rlo) and np.array_equal(hi, rhi), (T, lo, rlo, hi, rhi)
                    assert (hi - lo >= 2).all()
                    n += 1
    assert n >= 12 * 6
    # the camera 40 blocks from the origin in negative coordinates looks along -y: its box lies below -40
    lay = capi.depth_image_layout(width=48, height=32, encoding=capi.DEPTH_16UC1)
    rc, lo, hi = capi.projective_box(lay, cams[0].capi(capi), cfgs[0].capi(capi), _poses()[6], 0.1, 8)
    assert rc == capi.OK and (hi < -30).all() and hi[1] == -40 and lo[1] == -47


def test_the_box_holds_every_voxel_the_rules_update():
    """the restatement's own check of the header's claim, on every scene of the GPU test: a changed voxel's block is never
    on the box's outermost layer (the box is widened by one block: nothing is cut off)"""
    for name in S.CASES:
        img, cam, cfg, T, vs, vps = S.case(name)
        fr = P.integrate(P.Layer(vs, vps), T, img, cam, cfg)
        _, lo, hi = P.box(img.width, img.height, cam, cfg, T, vs, vps)
        blocks = fr.voxel[fr.branch >= P.UPDATED] // vps
        assert (blocks > lo).all() and (blocks < hi).all(), name


def test_the_box_refuses(capi):
    lay, cam, cfg = capi.depth_image_layout(width=48, height=32, encoding=capi.DEPTH_16UC1), P.Camera(**S.CAMERA), S.config(0.1)
    box = lambda *a: capi.projective_box(*a)[0]
    assert box(lay, cam.capi(capi), cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.OK
    assert box(None, cam.capi(capi), cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.ERR_INVALID
    assert box(lay, None, cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.ERR_INVALID
    assert box(lay, cam.capi(capi), None, S.IDENTITY, 0.1, 8) == capi.ERR_INVALID
    assert box(lay, cam.capi(capi, fx=0.0), cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.ERR_INVALID
    assert box(lay, cam.capi(capi, stride_u=0), cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.ERR_INVALID
    big = capi.depth_image_layout(width=48, height=32, encoding=capi.DEPTH_16UC1, is_bigendian=1)
    assert box(big, cam.capi(capi), cfg.capi(capi), S.IDENTITY, 0.1, 8) == capi.ERR_UNSUPPORTED
    bad = S.IDENTITY.copy()
    bad[5] = np.nan
    assert box(lay, cam.capi(capi), cfg.capi(capi), bad, 0.1, 8) == P.box(48, 32, cam, cfg, bad, 0.1, 8)[0] == capi.ERR_INVALID
    assert box(lay, cam.capi(capi), cfg.capi(capi), S.IDENTITY, 0.0, 8) == capi.ERR_INVALID
    assert box(lay, cam.capi(capi), cfg.capi(capi), S.IDENTITY, 0.1, 12) == capi.ERR_INVALID
    unbounded = S.config(0.1, max_ray_length_m=float("inf"))
    assert box(lay, cam.capi(capi), unbounded.capi(capi), S.IDENTITY, 0.1, 8) == P.box(48, 32, cam, unbounded, S.IDENTITY, 0.1, 8)[0] \
        == capi.ERR_UNSUPPORTED
    assert box(lay, cam.capi(capi, max_depth_m=3.0), unbounded.capi(capi), S.IDENTITY, 0.1, 8) == capi.OK      # (the gate bounds it)
    wide = capi.depth_image_layout(width=1 << 24, height=1, encoding=capi.DEPTH_16UC1)
    assert box(wide, cam.capi(capi), cfg.capi(capi), S.IDENTITY, 0.1, 8) == P.box(1 << 24, 1, cam, cfg, S.IDENTITY, 0.1, 8)[0] \
        == capi.ERR_UNSUPPORTED
    far = S.IDENTITY.copy()
    far[4] = 1e12
    assert box(lay, cam.capi(capi), cfg.capi(capi), far, 0.1, 8) == P.box(48, 32, cam, cfg, far, 0.1, 8)[0] == capi.ERR_UNSUPPORTED


def test_new_symbols_are_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "voxgraph_amd.h")).read()
    declared = set(re.findall(r"VGX_API\s+[\w\s\*]+?\b(vgx_\w+)\s*\(", header))
    lib = os.path.join(ROOT, "voxgraph_amd", "lib", "libvoxgraph_amd.so")
    exported = {line.split()[-1] for line in subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True).splitlines() if line}
    for name in NEW:
        assert name in declared and name in exported and name in capi.SIGNATURES, name
        assert getattr(capi.load(), name).argtypes == capi.SIGNATURES[name][1]
    assert "typedef struct vgx_projective_counts" in header and C.sizeof(capi.ProjectiveCounts) == 40
    section = header[header.index("Projective depth-image integration"):header.index("typedef struct vgx_projective_counts")]
    for field in ("use_sparsity_compensation_factor", "start_voxel_subsampling_factor", "enable_anti_grazing", "deterministic",
                  "integration_order"):
        assert field in section                                           # (stated as not read)


def test_null_handles_and_bad_frames_are_refused_without_a_device(capi):
    """no context exists here: a NULL integrator is refused, and a frame vgx_depth_image_check refuses is refused with the
    check's own code before the handle is looked at (the frame is checked first)"""
    lib, T = capi.load(), S.IDENTITY.copy()
    Tp = T.ctypes.data_as(capi.f32p)
    buf = np.zeros(6 * 4 * 4 + 64, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    cases = [({}, {}, 0, 0), (dict(encoding=2), {}, 0, 0), (dict(color_kind=6), {}, 0, 0), (dict(row_step=11), {}, 0, 0),
             (dict(color_row_step=17), {}, 0, 0), ({}, {}, -1, 0), ({}, {}, 0, -1), ({}, dict(fx=0.0), 0, 0),
             ({}, dict(fy=float("nan")), 0, 0), ({}, dict(cx=float("inf")), 0, 0), ({}, dict(depth_unit_m=0.0), 0, 0),
             ({}, dict(min_depth_m=float("nan")), 0, 0), ({}, dict(min_depth_m=-1.0), 0, 0), ({}, dict(min_depth_m=2.0, max_depth_m=1.0), 0, 0),
             ({}, dict(stride_u=0), 0, 0), ({}, dict(stride_v=-1), 0, 0), (dict(is_bigendian=1), {}, 0, 0),
             (dict(width=1 << 16, height=1 << 15, row_step=1 << 17, color_row_step=3 << 16), {}, 0, 0)]
    codes = set()
    for lay_kw, cam_kw, dn, cn in cases:
        l = dict(width=6, height=4, row_step=14, encoding=capi.DEPTH_16UC1, color_kind=capi.IMAGE_COLOR_RGB8, color_row_step=19)
        l.update(lay_kw)
        c = dict(fx=5.0, fy=5.1, cx=2.7, cy=1.4)
        c.update(cam_kw)
        layout, camera = capi.depth_image_layout(**l), capi.depth_camera(**c)
        need = (layout.height - 1) * layout.row_step + layout.width * 2 + dn
        cneed = (layout.height - 1) * layout.color_row_step + layout.width * 3 + cn
        want = capi.depth_image_check(layout, camera, need, cneed)
        assert (want == capi.OK) == (not lay_kw and not cam_kw and dn == 0 and cn == 0)
        for fn in (lib.vgx_tsdf_integrate_depth_image, lib.vgx_tsdf_integrate_depth_image_device):
            counts = capi.ProjectiveCounts()
            got = fn(None, Tp, C.byref(layout), C.byref(camera), p, need, p, cneed, C.byref(counts))
            assert got == (want if want != capi.OK else capi.ERR_INVALID), (lay_kw, cam_kw, dn, cn, got, want)
        codes.add(want)
    assert codes == {capi.OK, capi.ERR_INVALID, capi.ERR_UNSUPPORTED}
    for fn in (lib.vgx_tsdf_integrate_depth_image, lib.vgx_tsdf_integrate_depth_image_device):
        assert fn(None, Tp, None, None, None, 0, None, 0, None) == capi.ERR_INVALID


def test_the_gpu_scenes_reach_every_branch():
    """what tests/test_projective_gpu.py integrates, in the restatement alone: no GPU test passes on nothing"""
    seen, dropped_off, new, held = set(), 0, 0, 0
    for name in S.CASES:
        img, cam, cfg, T, vs, vps = S.case(name)
        L = P.Layer(vs, vps)
        first, second = P.integrate(L, T, img, cam, cfg), P.integrate(L, T, img, cam, cfg)
        for fr in (first, second):
            seen |= set(np.unique(fr.branch).tolist())
            dropped_off += int(fr.dropped_off.sum())
        new, held = new + first.new_blocks, held + second.held_blocks
        assert first.counts["n_updates"] == int((first.branch >= P.UPDATED).sum()) > 1000
        assert len(L.block_index) == first.new_blocks and second.new_blocks == 0 and second.held_blocks == first.new_blocks
    # updated, carved, cleared, behind the surface, no pixel, invalid depth -- and the refusals of carving and clearing
    assert {P.UPDATED, P.CARVED, P.CLEARED, P.BEHIND, P.NO_PIXEL, P.INVALID_DEPTH, P.CARVE_REFUSED, P.CLEAR_REFUSED} <= seen
    assert dropped_off > 1000 and new > 100 and held > 100
    # every kind of hole is in the 32FC1 frame, zeros in the 16UC1 frame
    z32 = S.frame(P.DEPTH_32FC1)[0].z(P.Camera(**S.CAMERA))
    assert np.isnan(z32).any() and (z32 == 0).any() and (z32 == -1).any() and np.isposinf(z32).any() and (z32 > 4.3).any()
    assert (S.frame(P.DEPTH_16UC1)[0].z(P.Camera(**S.CAMERA)) == 0).sum() > 20
