"""Shared helpers for the parity tests (test infrastructure)."""
import hashlib
import json
import os

import numpy as np

from oracle import pyoracle as orc
from oracle import ref_reg

# north_star tolerance: 1e-4 relative on residuals/Jacobians.  Residuals
# legitimately cross zero, so "relative" is against max(|oracle|, FLOOR * ||oracle||_inf)
# (SURVEY.md 4.3).
REL_TOL = 1e-4
FLOOR = 1e-3


def assert_parity(got, want, what="", rel=REL_TOL, floor=FLOOR):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size == 0:
        return 0.0
    scale = np.maximum(np.abs(want), floor * np.abs(want).max())
    scale = np.maximum(scale, 1e-300)
    err = np.abs(got - want) / scale
    worst = float(err.max())
    assert worst <= rel, f"{what}: worst relative error {worst:.3e} at {int(err.argmax())}"
    return worst


def oracle_layer(sm, use_esdf=True):
    if use_esdf:
        return orc.Layer(sm.voxel_size, sm.vps, sm.block_index, sm.esdf_distance, sm.esdf_observed)
    return orc.Layer(sm.voxel_size, sm.vps, sm.block_index, sm.tsdf_distance,
                     (sm.tsdf_weight > 0).astype(np.uint8))


def oracle_points(sm, use_esdf=True, min_w=1.0, max_d=0.3):
    return orc.find_relevant_voxels(sm.voxel_size, sm.vps, sm.block_index, sm.tsdf_distance,
                                    sm.tsdf_weight, sm.esdf_distance if use_esdf else None,
                                    min_w, max_d)


def gpu_submap(capi, ctx, sm, submap_id=0):
    return capi.Submap(ctx, submap_id, sm.voxel_size, sm.vps, sm.block_index, sm.tsdf_distance,
                       sm.tsdf_weight, sm.esdf_distance, sm.esdf_observed)


# the reference's perturbation grid (config/registration_test_bench.yaml:9-13),
# scaled to the voxel size as in SURVEY.md 8d config 1
def test_bench_grid(voxel_size):
    s = voxel_size / 0.2
    out = []
    for x in (-0.6 * s, 0.0, 0.3 * s):
        for y in (-0.6 * s, 0.0, 0.3 * s):
            for z in (-0.6 * s, 0.0, 0.3 * s):
                for yaw in (-0.2, 0.0, 0.1):
                    out.append(np.array([x, y, z, yaw]))
    return out


def digest(a):
    """SHA-256 of an array's bits, -0 counted as +0 (np.array_equal's view of equality)"""
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a) + 0.0).tobytes()).hexdigest()


def summarize(v):
    """what a pin test compares: arrays by digest, everything else (bools, numbers, None, lists of them) by value"""
    if isinstance(v, np.ndarray):
        return digest(v)
    if isinstance(v, (list, tuple)):
        return [summarize(x) for x in v]
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    return v


class ReferenceOutputs:
    """The outputs of the reference's own source (oracle/_ref/libref_reg.so) that the pin tests hold the oracle to,
    stored in tests/golden/ref_outputs.json: array digests, and values where an output is an input of the oracle's side.
    Where the library exists every output is also computed live and must equal the stored one;
    VGX_RECORD_REF_OUTPUTS=1 (there) rewrites the stored ones instead (tests/golden/make_ref_golden.py says when)."""
    PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_outputs.json")

    def __init__(self):
        self.live = ref_reg.available()
        self.record = self.live and os.environ.get("VGX_RECORD_REF_OUTPUTS") == "1"
        with open(self.PATH) as f:
            self.stored = json.load(f)
        self.recorded = {}

    def get(self, key, compute):
        """the stored summary of output `key`; `compute()` returns the live output where the library exists"""
        if not self.live:
            assert key in self.stored, f"{key}: not in {os.path.basename(self.PATH)}"
            return self.stored[key]
        got = summarize(compute())
        if self.record:
            self.recorded[key] = got
        else:
            assert got == self.stored.get(key), f"{key}: the live reference no longer gives the stored output"
        return got

    def save(self):
        if self.recorded:
            with open(self.PATH) as f:
                stored = json.load(f)
            stored.update(self.recorded)
            with open(self.PATH, "w") as f:
                json.dump(stored, f, indent=0, sort_keys=True)
                f.write("\n")
