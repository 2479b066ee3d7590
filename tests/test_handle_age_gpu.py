"""Long-lived handles at the moments only age reaches (DESIGN.md "Handle age"): the epoch rollover of a TileChain at
2^30 - 1 launches, the wrap of its 32-bit ticket count, and the full reset of the two approximate hash sets at offset
10 000.  A suite run makes a few hundred launches per handle; the tooling library's age setters
(include/voxgraph_amd_bench.h) put a handle a launch or two before the moment, keeping the stale tile words real launches
left, and empty scans age the sets on both sides.  Every comparison is exact: the restatement or the oracle, and the same
call on a fresh handle, byte for byte."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as orc
from profiles import fuzz_beam_table as ZB
from profiles.fuzz_projective import on_device, same_layer
from tests import beam_table_ref as B
from tests import beam_table_scenes as BS
from tests import depth_image_ref as D
from tests import projective_ref as P
from tests import projective_scenes as PS
from tests import scan_msg_ref as R
from tests import scan_msg_scenes as S
from tests import scan_undistort_ref as U
from tests import scan_undistort_scenes as Z
from tests.test_tsdf_deterministic_gpu import _assert_layers_identical, _lidar_scan

pytestmark = pytest.mark.gpu
F = np.float32
MAX = (1 << 30) - 1            # kChainEpochMax (csrc/vgx_chain_clock.h)
WRAP = 1 << 32
FULL_RESET = 10000             # ApproxHashSet's full_reset_threshold [recalled]: kFullResetThreshold / ORC_FULL_RESET
POISON = (1 << 64) - 1


@pytest.fixture(scope="module")
def capi():
    from voxgraph_amd import capi as m
    m.load()
    assert m.CHAIN_EPOCH_MAX == MAX
    return m


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


# ---- the scan decode ---------------------------------------------------------------------------------------------

TIME = U.TimeField(U.TIME_UINT32, 20, 1e-9, 0.0)      # nanoseconds in the 4 bytes behind xyzi32's intensity
TILES = 68                                            # of tests/scan_msg_scenes.aged_pair: 69 077 points
DEPTH_W, DEPTH_H, DEPTH_TILES = 320, 240, 75
VARIANTS = ["plain_host", "plain_device", "undistort_host", "undistort_device", "depth_image"]


def _as_bytes(pts, rgba):
    return np.ascontiguousarray(pts, F).view(np.uint8).tobytes(), np.ascontiguousarray(rgba).view(np.uint8).tobytes()


@pytest.fixture(scope="module")
def inputs():
    """A and B of every decode variant with what the restatements say of them, computed once and left unchanged:
    variant -> [(arguments, expected result)] for A, B.  A result is (stats, undistort stats, depth stats, point bytes,
    colour bytes)."""
    pair = S.aged_pair(0)
    msgs = []
    for k, m in enumerate(pair):
        assert (m.n + 1023) // 1024 == TILES and m.n % 1024 != 0
        rng = np.random.default_rng(50 + k)
        Z.put_time(m, TIME, Z.raw_times(TIME, rng.uniform(0.0, 0.1, m.n)))
        kt, kT = Z.knots(m, TIME, 5, seed=50 + k)
        msgs.append((m, kt, kT))
    out = {v: [] for v in VARIANTS}
    for m, kt, kT in msgs:
        pts, rgba, kept = R.decode(m)
        assert 0.6 * m.n < len(kept) < 0.8 * m.n
        plain = ((len(pts), m.n - len(pts)), (0, 0, 0), (0, 0, 0, 0)) + _as_bytes(pts, rgba)
        upts, urgba, _, st = U.decode(m, TIME, kt, kT)
        assert st["clamped"] > 1000 and st["not_finite"] == m.n - len(kept)
        und = ((len(upts), st["not_finite"] + st["bad_time"] + st["overflowed"]), (st["bad_time"], st["overflowed"], st["clamped"]),
               (0, 0, 0, 0)) + _as_bytes(upts, urgba)
        for v in ("plain_host", "plain_device"):
            out[v].append(((m,), plain))
        for v in ("undistort_host", "undistort_device"):
            out[v].append(((m, kt, kT), und))
    cam = D.camera_for(DEPTH_W, DEPTH_H, min_depth_m=D.MIN_DEPTH, max_depth_m=D.MAX_DEPTH)
    for seed in (1, 2):
        img = D.planted_image(DEPTH_W, DEPTH_H, D.DEPTH_16UC1, seed=seed)
        pts, rgba, _, st = D.decode(img, cam)
        assert st["invalid"] > 1000 and st["out_of_range"] > 1000 and (st["candidates"] + 1023) // 1024 == DEPTH_TILES
        want = ((len(pts), D.dropped(st)), (0, 0, 0), (st["candidates"], st["invalid"], st["out_of_range"], st["overflowed"]))
        out["depth_image"].append(((img, cam), want + _as_bytes(pts, rgba)))
    # every tile's sum differs between A and B: the number kept of every 1024 candidates
    ka, kb = (np.add.reduceat(np.isin(np.arange(m.n), R.decode(m)[2]), np.arange(0, m.n, 1024)) for m, _, _ in msgs)
    assert (ka != kb).mean() > 0.9 and not np.array_equal(np.cumsum(ka), np.cumsum(kb))
    return out


def _decode(capi, scan, variant, args):
    """one decode -> everything the call and the handle report of it"""
    if variant == "depth_image":
        img, cam = args
        stats = scan.decode_depth_image(img.layout(capi), cam.capi(capi), img.depth, img.color)
    else:
        m = args[0]
        held = None
        if variant.endswith("_device"):
            held, addr = on_device(m.data, 0)
        if variant == "plain_host":
            stats = scan.decode_msg(m.layout(capi), m.data)
        elif variant == "plain_device":
            stats = scan.decode_msg_device(m.layout(capi), addr, len(m.data))
        elif variant == "undistort_host":
            stats = scan.decode_undistorted(m.layout(capi), m.data, TIME.capi(capi), args[1], args[2])
        else:
            stats = scan.decode_undistorted_device(m.layout(capi), addr, len(m.data), TIME.capi(capi), args[1], args[2])
        del held
    assert scan.stats() == stats
    return (stats, scan.undistort_stats(), scan.depth_stats()) + _as_bytes(*scan.download())


def _differs(got, want):
    """the first field of a decode result that differs, or None"""
    for name, g, w in zip(("stats", "undistort stats", "depth stats", "points", "colours"), got, want):
        if g != w:
            return name if isinstance(g, bytes) else (name, g, w)
    return None


@pytest.mark.parametrize("variant", VARIANTS)
def test_scan_decode_across_the_epoch_rollover(capi, ctx, inputs, variant):
    """two real launches with A leave the tile words tagged 1 and 2 with status 2; from Max - 1 the three launches with B
    run at Max, then clear and 1, then 2 -- where the words would still read as A's sums had they not been cleared"""
    (args_a, want_a), (args_b, want_b) = inputs[variant]
    tiles = DEPTH_TILES if variant == "depth_image" else TILES
    old, new = capi.Scan(ctx), capi.Scan(ctx)
    try:
        for k in range(2):
            assert _differs(_decode(capi, old, variant, args_a), want_a) is None
            assert old.get_age() == (k + 1, (k + 1) * tiles)
        old.set_age(MAX - 1, 2 * tiles)
        assert old.get_age() == (MAX - 1, 2 * tiles)
        fresh = _decode(capi, new, variant, args_b)
        assert _differs(fresh, want_b) is None and new.get_age() == (1, tiles)
        for k, epoch in enumerate((MAX, 1, 2)):
            got = _decode(capi, old, variant, args_b)
            assert _differs(got, want_b) is None, (epoch, _differs(got, want_b))
            assert _differs(got, fresh) is None
            assert old.get_age() == (epoch, (3 + k) * tiles)
    finally:
        old.destroy()
        new.destroy()


def test_scan_decode_rollover_with_words_a_smaller_message_never_rewrote(capi, ctx, inputs):
    """Launches of one size rewrite every tile word, so in the test above no word still carries an old launch's tag when
    its epoch comes round again.  Here it would: A twice (all 68 words tagged 2, status 2), then a one-tile message at Max
    and at 1 -- the launch that clears -- and B at 2.  Without the clear, words 1 .. 67 still say "epoch 2, the sum up to
    here" with A's sums, and a tile of B that looks back before its neighbour has published takes them."""
    (args_a, want_a), (args_b, want_b) = inputs["plain_host"]
    small = S.small("xyzi32", 2)
    pts, rgba, _ = R.decode(small)
    want_small = ((len(pts), small.n - len(pts)), (0, 0, 0), (0, 0, 0, 0)) + _as_bytes(pts, rgba)
    assert small.n <= 1024
    old = capi.Scan(ctx)
    try:
        for k in range(2):
            assert _differs(_decode(capi, old, "plain_host", args_a), want_a) is None
        old.set_age(MAX - 1, 2 * TILES)
        for epoch in (MAX, 1):
            assert _differs(_decode(capi, old, "plain_host", (small,)), want_small) is None
            assert old.get_age()[0] == epoch
        got = _decode(capi, old, "plain_host", args_b)
        assert _differs(got, want_b) is None, _differs(got, want_b)
        assert old.get_age() == (2, 3 * TILES + 2)
    finally:
        old.destroy()


def test_scan_decode_with_the_ticket_wrap_inside_a_launch(capi, ctx, inputs):
    """tickets 2^32 - 30: workgroups 0 .. 29 of the 68 take theirs before the wrap, 30 .. 67 after it"""
    (args_a, want_a), (args_b, want_b) = inputs["plain_host"]
    old, new = capi.Scan(ctx), capi.Scan(ctx)
    try:
        assert _differs(_decode(capi, old, "plain_host", args_a), want_a) is None
        old.set_age(1, WRAP - 30)
        fresh = _decode(capi, new, "plain_host", args_b)
        assert _differs(fresh, want_b) is None
        for k in range(2):
            got = _decode(capi, old, "plain_host", args_b)
            assert _differs(got, want_b) is None and _differs(got, fresh) is None, k
        assert old.get_age() == (3, (WRAP - 30 + 2 * TILES) % WRAP) and old.get_age()[1] == 106
        # ... and the undistorting decode and a depth image on the handle that has wrapped
        (args_u, want_u), (args_d, want_d) = inputs["undistort_host"][0], inputs["depth_image"][1]
        assert _differs(_decode(capi, old, "undistort_host", args_u), want_u) is None
        assert _differs(_decode(capi, old, "depth_image", args_d), want_d) is None
        assert old.get_age() == (5, 106 + TILES + DEPTH_TILES)
    finally:
        old.destroy()
        new.destroy()


# ---- projective integration ----------------------------------------------------------------------------------------

PROJ_VS, PROJ_VPS = 0.1, 8


def _snapshot(layer):
    return tuple(np.array(a) for a in layer.download())


@pytest.fixture(scope="module")
def frames():
    """five frames from moving poses into one layer, for a depth camera and for a beam-table LiDAR, with the restatement's
    counts and layer after every frame (computed once): kind -> [(frame arguments, counts, layer arrays)]"""
    out = {"depth_image": [], "beam_table": []}
    cfg, ref = PS.config(PROJ_VS), P.Layer(PROJ_VS, PROJ_VPS)
    for k in range(5):
        T = PS.pose(PS.quat([0, 1, 0], 0.35 * k - 0.7), [0.15 * k - 0.3, 0.05 * k, 0.1 * k])
        img, cam = PS.frame(P.DEPTH_16UC1 if k % 2 == 0 else P.DEPTH_32FC1, T, P.COLOR_RGB8)
        want = P.integrate(ref, T, img, cam, cfg)
        out["depth_image"].append(((T, img, cam), want.counts, _snapshot(ref)))
    m, cfg, ref = BS.MODELS["64x8"], BS.config(PROJ_VS), B.Layer(PROJ_VS, PROJ_VPS)
    for k in range(5):
        T = BS.pose(BS.quat([0, 0, 1], 0.3 * k), [0.45 * k - 0.9, 0.25 * k - 0.6, 0.08 * k - 0.2])
        pts, rgba = BS.scan(m, T, seed=10 + k)
        want = B.integrate(ref, T, B.build(m, pts, rgba), cfg)
        out["beam_table"].append(((T, m, pts, rgba), want.counts, _snapshot(ref)))
    return out


class ProjRig:
    def __init__(self, capi, ctx, kind):
        self.capi, self.ctx, self.kind = capi, ctx, kind
        cfg = (PS if kind == "depth_image" else BS).config(PROJ_VS)
        self.layer = capi.TsdfLayer(ctx, PROJ_VS, PROJ_VPS)
        self.integ = capi.FastTsdfIntegrator(ctx, cfg.capi(capi), self.layer)
        self.image = capi.RangeImage(ctx) if kind == "beam_table" else None

    def frame(self, args):
        if self.kind == "depth_image":
            T, img, cam = args
            return self.integ.integrate_depth_image(T, img.layout(self.capi), cam.capi(self.capi), img.depth, img.color)
        T, m, pts, rgba = args
        ZB.build(self.capi, self.ctx, self.image, m, pts, rgba, True)
        return self.integ.integrate_range_image(T, self.image)

    def close(self):
        if self.image:
            self.image.destroy()
        self.integ.destroy()
        self.layer.destroy()


def _projective_frames(rig, frames, first, last):
    """frames first .. last - 1 against the restatement: counts, and the layer byte for byte, block order included"""
    for k in range(first, last):
        args, want, layer = frames[k]
        got = rig.frame(args)
        assert got == want, (k, got, want)
        # the shapes the issue asks for, from the returned counts: past one look-back window, and new blocks every frame
        assert got["n_candidate_blocks"] >= 65 and got["n_new_blocks"] > 0, (k, got)
        assert same_layer(rig.layer.download(), layer) is None, (k, same_layer(rig.layer.download(), layer))


@pytest.mark.parametrize("kind", ["depth_image", "beam_table"])
def test_projective_integration_across_the_epoch_rollover(capi, ctx, frames, kind):
    rig = ProjRig(capi, ctx, kind)
    try:
        _projective_frames(rig, frames[kind], 0, 2)
        tickets = sum(f[1]["n_candidate_blocks"] for f in frames[kind][:2])
        assert rig.integ.get_projective_age() == (2, tickets)
        rig.integ.set_projective_age(MAX - 1, tickets)
        for k, epoch in ((2, MAX), (3, 1), (4, 2)):
            _projective_frames(rig, frames[kind], k, k + 1)
            tickets += frames[kind][k][1]["n_candidate_blocks"]
            assert rig.integ.get_projective_age() == (epoch, tickets)
    finally:
        rig.close()


@pytest.mark.parametrize("kind", ["depth_image", "beam_table"])
def test_projective_integration_with_the_ticket_wrap_inside_a_frame(capi, ctx, frames, kind):
    rig = ProjRig(capi, ctx, kind)
    try:
        _projective_frames(rig, frames[kind], 0, 2)
        candidates = [f[1]["n_candidate_blocks"] for f in frames[kind]]
        rig.integ.set_projective_age(2, WRAP - candidates[2] // 2)
        _projective_frames(rig, frames[kind], 2, 5)
        assert rig.integ.get_projective_age() == (5, (WRAP - candidates[2] // 2 + sum(candidates[2:])) % WRAP)
    finally:
        rig.close()


# ---- the reproducible mode's chained launches and sweeps -------------------------------------------------------------

def _yawed(k, origin):
    """scan k of a moving, turning sensor: (pose, sensor-frame points)"""
    pts = _lidar_scan(512, 32, 70 + k, origin=origin.astype(np.float64))
    yaw = 0.15 * k
    c, s = np.cos(-yaw), np.sin(-yaw)
    pts = np.stack([c * pts[:, 0] - s * pts[:, 1], s * pts[:, 0] + c * pts[:, 1], pts[:, 2]], 1).astype(F)
    return np.r_[np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)], F), origin].astype(F), pts


@pytest.mark.parametrize("merged", [False, True], ids=["fast", "merged"])
def test_reproducible_mode_with_the_rollover_inside_a_scan(capi, ctx, merged):
    """the scratch's epoch set to Max - 3 after one scan.  The fast integrator makes tens of chained launches and sweeps a
    scan: the next scan takes Max - 2 .. Max, the words are cleared between two launches queued on the stream, and its later
    launches and sweeps run at 1, 2, ...  The merged integrator makes two chained launches a scan (group heads, ray offsets):
    its next scan takes Max - 2 and Max - 1, the one after it Max, then the clear and 1 -- the rollover between the two."""
    vs, vps = 0.2, 16
    ol, gl = orc.TsdfLayer(vs, vps), capi.TsdfLayer(ctx, vs, vps)
    oi = orc.FastTsdfIntegrator(orc.voxgraph_tsdf_config(), ol)
    gi = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), gl)
    rng = np.random.default_rng(8)
    rolled = []
    try:
        with pytest.raises(capi.VgxError):
            gi.get_reproducible_age()                       # no scratch yet
        for k in range(3):
            T, pts = _yawed(k, np.array([0.35 * k - 1.0, -0.22 * k + 0.5, 0.03 * k], F))
            col = rng.integers(0, 256, (len(pts), 4)).astype(np.uint8)
            if k == 1:
                per_scan = gi.get_reproducible_age()        # launches of the first scan
                assert (per_scan == 2) if merged else (4 < per_scan < 1000), per_scan
                gi.set_reproducible_age(MAX - 3)
            before = gi.get_reproducible_age() if k else 0
            if merged:
                a, b = oi.integratePointCloudMerged(T, pts, col), gi.integratePointCloudMerged(T, pts, col)
            else:
                a, b = oi.integratePointCloud(T, pts, col), gi.integratePointCloud(T, pts, col)
            assert a == b > 10000, (k, a, b)
            _assert_layers_identical(ol, gl, f"scan {k}")
            after = gi.get_reproducible_age()
            assert 1 <= after <= MAX
            if after < before:
                rolled.append((k, before, after))
        # the getter reads less after the scan the rollover fell into than before it, and that scan began before Max
        assert rolled == ([(2, MAX - 1, 1)] if merged else [(1, MAX - 3, rolled[0][2])]), rolled
        assert 1 <= rolled[0][2] < 1000
        assert gl.stats()[1] == 0
    finally:
        gi.destroy()
        gl.destroy()


# ---- the full reset of the two approximate sets ----------------------------------------------------------------------

ORIGIN = np.array([0.005, 0.005, 0.005], F)       # inside voxel (0, 0, 0) and inside start cell (0, 0, 0): the index whose hash is 0


def _reset_scan(k):
    """a LiDAR scan from ORIGIN (identity rotation) plus one return in start cell (0, 0, 0), 0.156 m away: a cast ray"""
    pts = _lidar_scan(512, 32, 90 + k, origin=ORIGIN.astype(np.float64))
    planted = (np.array([[0.095, 0.095, 0.095]], F) - ORIGIN).astype(F)
    return np.r_[np.array([1, 0, 0, 0], F), ORIGIN].astype(F), np.concatenate([pts, planted]).astype(F)


def _voxel_000_weight(layer):
    bi, _, w, _ = layer.download()
    row = np.flatnonzero((bi == 0).all(1))
    return float(w[row[0]].reshape(-1)[0]) if len(row) else 0.0


def _sets_equal(oi, gi):
    """both sets and both offsets equal the oracle's -> (oracle's start set, observed set, offsets)"""
    os_, oo, ooff = oi.download_sets()
    gs, go, goff = gi.download_sets()
    assert goff[:2] == ooff, (goff, ooff)
    assert np.array_equal(gs, os_), ("start set", int((gs != os_).sum()))
    assert np.array_equal(go, oo), ("observed set", int((go != oo).sum()))
    return os_, oo, ooff


@pytest.mark.parametrize("every", [1, 3])
def test_full_reset_of_the_sets_equals_the_oracles(capi, ctx, every):
    """clear_checks_every_n_frames = every: scan s carries the offset (s // every) mod 10 000.  Two real scans, empty scans
    (both sides count a scan before they look at n) up to offset 9 998, then real scans from the first one at 9 999 over
    the full reset to the first one at 1."""
    vs, vps = 0.2, 16
    ol, gl = orc.TsdfLayer(vs, vps), capi.TsdfLayer(ctx, vs, vps)
    oi = orc.FastTsdfIntegrator(orc.voxgraph_tsdf_config(clear_checks_every_n_frames=every), ol)
    gi = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1, clear_checks_every_n_frames=every), gl)
    empty = np.zeros((0, 3), F)
    try:
        def real(s):
            T, pts = _reset_scan(s % 7)
            a, b = oi.integratePointCloud(T, pts), gi.integratePointCloud(T, pts)
            assert a == b > 0, (s, a, b)
            _assert_layers_identical(ol, gl, f"scan {s}")
            start, observed, offsets = _sets_equal(oi, gi)
            assert offsets == ((s // every) % FULL_RESET,) * 2, (s, offsets)
            return start, observed
        first, last = (FULL_RESET - 1) * every, (FULL_RESET + 1) * every
        T0 = _reset_scan(0)[0]
        for s in range(1, first):
            if s <= 2:
                real(s)
            else:
                oi.integratePointCloud(T0, empty)
                gi.integratePointCloud(T0, empty, count=False)
        start, observed, offsets = _sets_equal(oi, gi)
        assert offsets == (FULL_RESET - 2,) * 2
        assert (start != 0).sum() > 1000 and (observed != 0).sum() > 10000       # the real scans' entries are still there
        for s in range(first, last + 1):
            before = _voxel_000_weight(ol)
            start, observed = real(s)
            if s == FULL_RESET * every:
                # the scan that reset: nothing older is left, and the index whose hash is 0 -- a start cell and an observed
                # voxel of this scan, value 0 + offset 0 -- was NOT found present in the zeroed slot 0: the poison's case
                assert _voxel_000_weight(ol) > before
                assert start[0] in (0, POISON) and observed[0] in (0, POISON)
                assert start[0] == 0 and observed[0] == 0                        # (overwritten with the oracle's value)
        assert gl.stats()[1] == 0
    finally:
        gi.destroy()
        gl.destroy()


def test_a_racing_scan_right_after_a_full_reset_is_a_legal_interleaving(capi, ctx):
    """racing mode: two real scans, empty scans to offset 9 999, then one traced scan -- it resets the sets first.  Replayed
    against the sets as the reset must leave them (zeros, slot 0 poisoned) and the downloaded offsets (0, 0)."""
    vs, vps = 0.2, 16
    az, el = np.meshgrid(np.linspace(-np.pi, np.pi, 256, endpoint=False) + (2 * np.pi / 256) / 3.0, np.linspace(-0.3, 0.3, 12) + 0.004)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], -1).reshape(-1, 3)
    lo, hi = np.array([-4.0, -3.0, -1.0]), np.array([4.5, 3.5, 2.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, hi / d, np.where(d < 0, lo / d, np.inf)).min(1)
    pts = (d * t[:, None]).astype(F)
    assert not (pts == 0).any()                  # (no ray with a zero component: oracle/PIN.md item 2)
    T = np.array([1, 0, 0, 0, 0.1, -0.05, 0.02], F)
    layer = capi.TsdfLayer(ctx, vs, vps)
    integ = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(clear_checks_every_n_frames=1), layer)
    try:
        for s in range(1, FULL_RESET):
            if s <= 2:
                assert integ.integratePointCloud(T, pts) > 0
            else:
                integ.integratePointCloud(T, np.zeros((0, 3), F), count=False)
        integ.set_event_trace(4 << 20)
        s0, o0, state = integ.download_sets()
        assert state[:2] == (FULL_RESET - 1,) * 2 and (s0 != 0).sum() > 100 and (o0 != 0).sum() > 1000
        cleared = np.zeros(1 << 20, np.uint64)
        cleared[0] = POISON
        layer0 = layer.download()
        n = integ.integratePointCloud(T, pts)
        trace, lost = integ.read_event_trace()
        s1, o1, (off_s, off_o, _) = integ.download_sets()
        assert (off_s, off_o) == (0, 0) and lost == 0
        rep = orc.tsdf_replay_check(orc.voxgraph_tsdf_config(clear_checks_every_n_frames=1), vs, vps, T, pts, None, False,
                                    (off_s, off_o), (cleared, cleared.copy()), (s1, o1), layer0, layer.download(), trace)
        assert rep["errors"] == 0, rep["first_error"]
        assert rep["required_updates"] == rep["fold_records"] == n > 0
    finally:
        integ.destroy()
        layer.destroy()


# ---- refusals ----------------------------------------------------------------------------------------------------------

def _refused(ctx, rc, text):
    from voxgraph_amd import capi
    msg = ctx.lib.vgx_last_error(ctx.h).decode()
    assert rc == capi.ERR_INVALID and text in msg, (rc, msg)


def test_refused_setters_change_nothing(capi, ctx, inputs, frames):
    lib = ctx.lib
    (args_a, want_a), (args_b, want_b) = inputs["plain_host"]
    scan = capi.Scan(ctx)
    rig = ProjRig(capi, ctx, "depth_image")
    gl = capi.TsdfLayer(ctx, 0.2, 16)
    gi = capi.FastTsdfIntegrator(ctx, capi.voxgraph_tsdf_config(deterministic=1), gl)
    e, t = C.c_int64(), C.c_int64()
    try:
        # handles that have not launched: there is no ticket word and no scratch
        _refused(ctx, lib.vgx_scan_set_age(scan.h, 5, 5), "vgx_scan_set_age: the scan has not decoded anything yet")
        _refused(ctx, lib.vgx_tsdf_integrator_set_projective_age(rig.integ.h, 5, 5), "no frame has been integrated yet")
        _refused(ctx, lib.vgx_tsdf_integrator_set_reproducible_age(gi.h, 5), "no reproducible or merged scan has been integrated yet")
        _refused(ctx, lib.vgx_tsdf_integrator_get_reproducible_age(gi.h, C.byref(e)), "no reproducible or merged scan has been integrated yet")
        assert scan.get_age() == (0, 0) and rig.integ.get_projective_age() == (0, 0)
        for fn in (lib.vgx_scan_set_age, lib.vgx_tsdf_integrator_set_projective_age):
            assert fn(None, 1, 1) == capi.ERR_INVALID
        assert lib.vgx_tsdf_integrator_set_reproducible_age(None, 1) == capi.ERR_INVALID
        assert lib.vgx_scan_get_age(None, C.byref(e), C.byref(t)) == capi.ERR_INVALID
        assert lib.vgx_tsdf_integrator_get_projective_age(None, C.byref(e), C.byref(t)) == capi.ERR_INVALID
        assert lib.vgx_tsdf_integrator_get_reproducible_age(None, C.byref(e)) == capi.ERR_INVALID
        # handles that have: values out of range
        assert _differs(_decode(capi, scan, "plain_host", args_a), want_a) is None
        _projective_frames(rig, frames["depth_image"], 0, 1)
        T, pts = _yawed(0, np.array([-1.0, 0.5, 0.0], F))
        ol = orc.TsdfLayer(0.2, 16)
        oi = orc.FastTsdfIntegrator(orc.voxgraph_tsdf_config(), ol)
        assert oi.integratePointCloud(T, pts) == gi.integratePointCloud(T, pts)
        ages = scan.get_age(), rig.integ.get_projective_age(), gi.get_reproducible_age()
        for epoch, tickets, text in ((-1, 0, "epoch is not in 0 .. 2^30 - 1"), (MAX + 1, 0, "epoch is not in 0 .. 2^30 - 1"),
                                     (1 << 40, 0, "epoch is not in 0 .. 2^30 - 1"), (1, -1, "tickets is not in 0 .. 2^32 - 1"),
                                     (1, WRAP, "tickets is not in 0 .. 2^32 - 1")):
            _refused(ctx, lib.vgx_scan_set_age(scan.h, epoch, tickets), "vgx_scan_set_age: " + text)
            _refused(ctx, lib.vgx_tsdf_integrator_set_projective_age(rig.integ.h, epoch, tickets),
                     "vgx_tsdf_integrator_set_projective_age: " + text)
            if tickets == 0:
                _refused(ctx, lib.vgx_tsdf_integrator_set_reproducible_age(gi.h, epoch), "vgx_tsdf_integrator_set_reproducible_age: " + text)
        assert (scan.get_age(), rig.integ.get_projective_age(), gi.get_reproducible_age()) == ages
        # ... and the handles' next results are what they would have been
        assert _differs(_decode(capi, scan, "plain_host", args_b), want_b) is None
        assert scan.get_age() == (2, 2 * TILES)
        _projective_frames(rig, frames["depth_image"], 1, 2)
        T, pts = _yawed(1, np.array([-0.65, 0.28, 0.03], F))
        assert oi.integratePointCloud(T, pts) == gi.integratePointCloud(T, pts)
        _assert_layers_identical(ol, gl, "after the refusals")
        # the ends of the ranges are accepted, and a getter takes NULL for what is not wanted
        scan.set_age(0, WRAP - 1)
        scan.set_age(MAX, 0)
        assert lib.vgx_scan_get_age(scan.h, None, None) == capi.OK and scan.get_age() == (MAX, 0)
        assert _differs(_decode(capi, scan, "plain_host", args_a), want_a) is None and scan.get_age() == (1, TILES)
    finally:
        gi.destroy()
        gl.destroy()
        rig.close()
        scan.destroy()
