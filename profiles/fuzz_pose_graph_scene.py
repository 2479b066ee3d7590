"""Scenes for profiles/fuzz_pose_graph.py, drawn from a seed and needing no device and no library: a matrix scene (a block
matrix for vgx_block_spd_solve / vgx_dense_spd_solve and their _many forms, with a bad pivot in one scene in six), a graph
scene (an edges-only pose graph with its solver options, ordering and covariance pairs) and a registration scene (a
constraint list, constant flags and edges over the ring of 12 submaps the driver builds once).

The classes follow the seed by a fixed schedule, not by a draw, so that a short range of seeds holds each of them: the
size classes have a period of 24 seeds, in which the `wide` class (280 - 330 block rows or nodes: a column with more than
16 tiles under its diagonal) comes twice; the pattern families and topologies cycle; bad pivots come in one matrix scene in
six (two variants of the clean matrix, one diagonal element replaced in each, their kinds cycling); two slots hold the
rank-deficient sub-class.  Everything else comes from numpy's generator seeded with (seed, a word per scene kind).

`structure_features` states, from the restated tile lists alone, which paths of the kernels a structure reaches;
tests/test_fuzz_pose_graph_cpu.py holds the suite's seeds to them."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import pose_graph_ref as ref  # noqa: E402
from tests import pose_graph_sparse_covariance_ref as scov  # noqa: E402
from tests import pose_graph_sparse_ref as sref  # noqa: E402

NODES_PER_TILE, TILE = sref.NODES_PER_TILE, sref.TILE
ORDERINGS = (sref.NATURAL, sref.RCM, sref.GIVEN)
FAMILIES = ("empty", "chain", "chain2", "random", "hub", "arrow", "band", "components", "relabelled")
# block rows of a matrix scene, by seed % 24
ROW_CLASSES = {"1": (1, 1), "15": (15, 15), "16": (16, 16), "17": (17, 17), "31-33": (31, 33), "48": (48, 48), "63-65": (63, 65),
               "100": (100, 100), "wide": (280, 330)}
ROW_SCHEDULE = ("31-33", "wide", "63-65", "100", "48", "15", "wide", "17", "31-33", "16", "63-65", "1",
                "1", "15", "16", "17", "31-33", "48", "63-65", "100", "31-33", "63-65", "48", "100")
M_VALUES = (1, 3, 4, 31, 32, 33, 64, 65, 100)
BAD_KINDS = ("nonpositive", "inf", "nan", "fill")
# nodes of a graph scene, by seed % 24: four of the 24 have a free part that fits one tile
NODE_CLASSES = {"1": (1, 1), "2": (2, 2), "5": (5, 5), "16-18": (16, 18), "32-34": (32, 34), "50": (50, 50), "64-66": (64, 66),
                "90": (90, 90), "130": (130, 130), "wide": (280, 330)}
NODE_SCHEDULE = ("32-34", "50", "64-66", "wide", "90", "32-34", "130", "50", "64-66", "wide", "32-34", "50",
                 "16-18", "2", "64-66", "5", "90", "1", "130", "32-34", "50", "64-66", "90", "32-34")
RANK_DEFICIENT_SLOTS = (4, 14)
TOPOLOGIES = ("tree", "tree_closures", "hub", "random", "components", "relabelled")
RADII = (1e-2, 1.0, 1e2, 1e4)
MATRIX_WORD, GRAPH_WORD, REG_WORD, PATTERN_WORD = 0x6d617478, 0x67726166, 0x72656773, 0x70617474


# ---- block patterns -------------------------------------------------------------------------------------------------
def pattern(rng, family, n, hub_fraction=None, hub_at=None):
    """-> sorted pairs (i, j), i > j, no repeats, over n block rows"""
    pairs = set()

    def join(a, b):
        if a != b:
            pairs.add((max(int(a), int(b)), min(int(a), int(b))))

    if n >= 2:
        if family in ("chain", "chain2"):
            for i in range(n - 1):
                join(i + 1, i)
            if family == "chain2":
                for i in range(n - 2):
                    join(i + 2, i)
        elif family == "random":
            for _ in range(int(rng.choice((0.5, 1.5, 4.0)) * n)):
                join(rng.integers(n), rng.integers(n))
        elif family == "hub":
            hub = int((0, n // 2, n - 1, rng.integers(n))[int(rng.integers(4))]) if hub_at is None else hub_at
            fraction = rng.uniform(0.3, 0.9) if hub_fraction is None else hub_fraction
            for i in np.flatnonzero(rng.random(n) < fraction):
                join(hub, i)
            if rng.random() < 0.5:
                for i in range(n - 1):
                    join(i + 1, i)
        elif family == "arrow":
            for i in range(1, n):
                join(i, 0)
        elif family == "band":
            for w in range(1, int(rng.integers(1, 4)) + 1):
                for i in range(n - w):
                    join(i + w, i)
            for _ in range(int(rng.integers(1, 5))):
                join(rng.integers(n), rng.integers(n))
        elif family == "components":
            cuts = sorted(set(rng.integers(1, n, int(rng.integers(1, 4))).tolist()))
            for lo, hi in zip([0] + cuts, cuts + [n]):
                members = [i for i in range(lo, hi) if rng.random() < 0.85]                   # the others stay isolated
                for a, b in zip(members, members[1:]):
                    join(a, b)
                for _ in range(len(members) // 8):
                    join(rng.choice(members), rng.choice(members))
        elif family == "relabelled":
            label = rng.permutation(n)
            for i in range(n - 1):
                join(label[i + 1], label[i])
    return sorted(pairs)


def pattern_case(k):
    """the k-th random structure of the host pattern sweep (tests/test_fuzz_pose_graph_cpu.py): -> (family, n, pairs as
    the library takes them: either direction, some repeated, some of a node with itself, given permutation)"""
    rng = np.random.default_rng([k, PATTERN_WORD])
    family = FAMILIES[k % len(FAMILIES)]
    lo, hi = ROW_CLASSES[ROW_SCHEDULE[(k // len(FAMILIES)) % len(ROW_SCHEDULE)]]
    n = int(rng.integers(lo, hi + 1))
    pairs = [p if rng.random() < 0.5 else p[::-1] for p in pattern(rng, family, n)]
    if pairs and rng.random() < 0.5:
        pairs += [pairs[int(i)] for i in rng.integers(len(pairs), size=3)]
    if rng.random() < 0.3:
        v = int(rng.integers(n))
        pairs.append((v, v))
    return family, n, pairs, rng.permutation(n)


# ---- what a structure reaches ---------------------------------------------------------------------------------------
def structure_features(n_block_rows, free_pairs, order):
    """-> (features: a set of names, h_keys, l_tiles) of the tile structure of `free_pairs` under `order`"""
    nf = 4 * n_block_rows
    h_keys, l_tiles = sref.tile_pattern(n_block_rows, free_pairs, order)
    nT = (n_block_rows + NODES_PER_TILE - 1) // NODES_PER_TILE
    feats = set()
    cols, rows = sref.columns_of(l_tiles), {}
    for I, J in l_tiles:
        if I != J:
            rows.setdefault(I, []).append(J)
    fill = {t for t in l_tiles if t not in h_keys}
    if fill:
        feats.add("pure_fill_tile")
    for K, (I, J), a, b in sref.update_triples(l_tiles):
        if (I, J) in fill and (a in fill or b in fill):
            feats.add("fill_of_fill")
        if nf % TILE and I == nT - 1:
            feats.add("partial_row_is_I_and_J" if J == nT - 1 else "partial_row_is_I_alone")
    for K in range(nT):
        below = len(cols[K]) - 1
        if K < nT - 1:                                                     # (the last column has nothing below it anyway)
            feats.add("empty_column" if below == 0 else "column_count_odd" if below % 2 else "column_count_even")
        if below > 16:
            feats.add("column_over_16_tiles")
        left = len(rows.get(K, ()))
        if left:
            feats.add("row_count_odd" if left % 2 else "row_count_even")
        if left > 16:
            feats.add("row_over_16_tiles")
    return feats, h_keys, l_tiles


def chunk_features(nf, l_tiles, place, pairs):
    """what the chunks of pg_solve_many_tiled_kernel do for the covariance pairs: a forward pass that starts past panel 0, a
    backward pass that skips a stored tile left of the panel of the lowest wanted row"""
    feats = set()
    _, _, unit_rows, chunks = scov.column_lists(place, pairs)
    for first_row, lowest in chunks:
        if first_row // TILE > 0:
            feats.add("forward_starts_past_panel_0")
        p_last = lowest // TILE
        if any(J < p_last <= I for I, J in l_tiles if I != J):
            feats.add("backward_skips_a_tile")
    return feats


# ---- matrix scenes --------------------------------------------------------------------------------------------------
def blocks_of(A, m):
    return np.array([A[4 * i:4 * i + 4, 4 * j:4 * j + 4] for i, j in zip(m["bi"], m["bj"])])


def arrow_matrix(d):
    """tests/test_pose_graph_sparse_gpu.py's arrow: 33 block rows, node 0 the identity, every other node d I with the block I
    towards node 0; the last node's pivot is d - 32, negative for d < 32 through the fill tile (2, 1) alone"""
    A = np.zeros((132, 132))
    A[:4, :4] = np.eye(4)
    for i in range(1, 33):
        A[4 * i:4 * i + 4, 4 * i:4 * i + 4] = d * np.eye(4)
        A[4 * i:4 * i + 4, :4] = A[:4, 4 * i:4 * i + 4] = np.eye(4)
    return A


def matrix_scene(seed):
    rng = np.random.default_rng([seed, MATRIX_WORD])
    cls = ROW_SCHEDULE[seed % len(ROW_SCHEDULE)]
    rows = int(rng.integers(ROW_CLASSES[cls][0], ROW_CLASSES[cls][1] + 1))
    family = FAMILIES[(seed + seed // len(ROW_SCHEDULE)) % len(FAMILIES)]
    bad_kinds = [BAD_KINDS[(seed // 6 + k) % len(BAD_KINDS)] for k in (0, 2)] if seed % 6 == 3 else []
    if cls == "wide" and rng.random() < 0.75:
        family, pairs = "hub", pattern(rng, "hub", rows, hub_fraction=0.8, hub_at=int(rng.integers(NODES_PER_TILE)))
    elif "fill" in bad_kinds:
        cls, rows, family, pairs = "31-33", 33, "arrow", pattern(rng, "arrow", 33)
    else:
        pairs = pattern(rng, family, rows)
    m = sref.block_matrix(rows, pairs, seed=seed)
    n = m["n"]
    sc = SimpleNamespace(seed=seed, size_class=cls, rows=rows, n=n, family=family, pairs=m["pairs"], bi=m["bi"], bj=m["bj"], A=m["A"],
                         b=m["b"], m=int(rng.choice(M_VALUES)), in_place=bool(rng.integers(2)), bad=[])
    d = float(rng.uniform(31.0, 32.0))
    if "fill" in bad_kinds:
        sc.A = arrow_matrix(d + 1.0)
    for kind in bad_kinds:                                                 # each variant: one diagonal element of the clean matrix replaced
        if kind == "fill":
            sc.bad.append(SimpleNamespace(kind="fill", row=128, A=arrow_matrix(d), last_tile=False))
            continue
        in_last = n % TILE != 0 and rng.random() < 0.5
        row = int(rng.integers(n - n % TILE, n)) if in_last else int(rng.integers(n))
        value = {"nonpositive": (0.0, -0.0, -1e6, -1e-300)[int(rng.integers(4))], "inf": np.inf, "nan": np.nan}[kind]
        A = sc.A.copy()
        A[row, row] = value
        sc.bad.append(SimpleNamespace(kind=kind, row=row, A=A, last_tile=bool(n % TILE and row >= n - n % TILE)))
    sc.values = blocks_of(sc.A, m)
    sc.B = rng.normal(0, 1, (n, sc.m))
    if sc.m >= 4:                                                          # a unit column, a zero column
        sc.B[:, 1] = np.eye(n)[:, int(rng.integers(n))]
        sc.B[:, 3] = 0.0
    sc.features, sc.h_keys, sc.l_tiles = structure_features(rows, sc.pairs, list(range(rows)))
    return sc


# ---- graph scenes ---------------------------------------------------------------------------------------------------
def _edges_of(rng, topology, n):
    """node pairs (a, b), a != b, in list order, with repeats and both directions"""
    if n < 2:
        return []
    pairs = []
    if topology in ("tree", "tree_closures"):
        pairs = [(int(rng.integers(k)), k) for k in range(1, n)]
        if topology == "tree_closures":
            pairs += [tuple(int(v) for v in rng.choice(n, 2, replace=False)) for _ in range(max(1, n // 10))]
    elif topology == "hub":
        hub = int((0, n // 2, n - 1, rng.integers(n))[int(rng.integers(4))])
        pairs = [(k, k + 1) for k in range(n - 1)]
        pairs += [(hub, int(k)) if i % 2 else (int(k), hub) for i, k in enumerate(np.flatnonzero(rng.random(n) < 0.4)) if k != hub]
    elif topology == "random":
        pairs = [(k, k + 1) for k in range(n - 1) if rng.random() < 0.9]
        pairs += [tuple(int(v) for v in rng.choice(n, 2, replace=False)) for _ in range(int(rng.choice((0.3, 1.0, 2.0)) * n))]
    elif topology == "components":
        cuts = sorted(set(rng.integers(1, n, int(rng.integers(1, 4))).tolist()))
        for lo, hi in zip([0] + cuts, cuts + [n]):
            pairs += [(k, k + 1) for k in range(lo, hi - 1)]
            pairs += [tuple(int(v) for v in lo + rng.choice(hi - lo, 2, replace=False)) for _ in range((hi - lo) // 8)]
    elif topology == "relabelled":
        label = rng.permutation(n)
        pairs = [(int(label[k]), int(label[k + 1])) for k in range(n - 1)]
    repeats = [pairs[int(i)] for i in rng.integers(len(pairs), size=min(4, len(pairs)))] if pairs else []
    return pairs + [p if rng.random() < 0.5 else p[::-1] for p in repeats]


def _components(n, joined):
    """-> the connected components as sorted arrays of nodes, by their lowest node"""
    root = list(range(n))

    def find(v):
        while root[v] != v:
            root[v] = root[root[v]]
            v = root[v]
        return v

    for a, b in joined:
        root[find(a)] = find(b)
    groups = {}
    for v in range(n):
        groups.setdefault(find(v), []).append(v)
    return sorted((np.array(g) for g in groups.values()), key=lambda g: g[0])


def graph_scene(seed):
    rng = np.random.default_rng([seed, GRAPH_WORD])
    slot = seed % len(NODE_SCHEDULE)
    cls = NODE_SCHEDULE[slot]
    n = int(rng.integers(NODE_CLASSES[cls][0], NODE_CLASSES[cls][1] + 1))
    topology = TOPOLOGIES[(seed + seed // len(NODE_SCHEDULE)) % len(TOPOLOGIES)]
    all_constant = cls == "2" and (seed // len(NODE_SCHEDULE)) % 2 == 0
    rank_deficient = slot in RANK_DEFICIENT_SLOTS
    lonely_kind = rank_deficient and (seed // len(NODE_SCHEDULE)) % 2 == 1  # a free node without an edge; else a component without a constant node
    if rank_deficient and not lonely_kind:
        topology = "components"
    joined = _edges_of(rng, topology, n)
    constant = np.zeros(n, np.int32)
    if all_constant:
        constant[:] = 1
    else:
        n_constant = int(rng.integers(1, max(1, n // 8) + 1))
        nodes = rng.choice(n, n_constant, replace=False)
        if rng.random() < 0.5 and 0 not in nodes:                          # node 0 is among them on some seeds only
            nodes[0] = 0
        constant[nodes] = 1
        if not rank_deficient:                                             # outside the scheduled sub-class no component floats
            for members in _components(n, joined):
                if not constant[members].any():
                    constant[int(rng.choice(members))] = 1
    lonely = None
    if lonely_kind:
        lonely = int(rng.choice(np.flatnonzero(constant == 0)))
        joined = [p for p in joined if lonely not in p]
    elif rank_deficient:                                                   # the constant nodes all in the first node's component
        reach = _components(n, joined)[0]
        constant[:] = 0
        constant[rng.choice(reach, max(1, min(len(reach) - 1, n // 8)), replace=False)] = 1
    constant = constant.tolist()
    # true poses on a circle, yaws once and a half around; observations with noise; full, odometry and closure information
    ang = np.linspace(0, 2 * np.pi, max(n, 2), endpoint=False)[:n]
    true = np.stack([3.0 * np.cos(ang) - 3.0, 3.0 * np.sin(ang), 0.02 * np.arange(n), 1.5 * ang], 1)
    true[:, 3] = [ref.normalize_angle(float(v)) for v in true[:, 3]]
    hard = rng.random() < 0.35                                             # tests/pose_graph_ref.mixed_graph's recipe for rejected steps
    yaw_information = 1.0 if hard else float(rng.choice((1.0, 2500.0)))
    translation_noise, yaw_noise = float(rng.choice((0.0, 0.01, 0.05))), float(rng.choice((0.0, 0.01, 0.05)))
    # a weakly tied node on some seeds: every edge of one free node of the lowest degree carries the sqrt-information 1e-4 I,
    # so that its diagonal of H lies below the 1e-6 that the damping clips to while its gradient does not vanish
    weak = None
    degree = np.bincount(np.asarray(joined, int).ravel(), minlength=n) if joined else np.zeros(n, int)
    candidates = [v for v in range(n) if not constant[v] and degree[v] > 0]
    if candidates and n >= 5 and rng.random() < 0.3:
        weak = min(candidates, key=lambda v: (degree[v], v))
    edges = []
    for a, b in joined:
        kind = int(rng.integers(3))
        info = (ref.INFO_ODOMETRY, ref.INFO_LOOP_CLOSURE, ref.INFO_LOOP_CLOSURE)[kind][:3] + (yaw_information,)
        _, _, t, yaw, S = ref.relative_edge(a, b, true[a], true[b], info)
        t = [v + rng.normal(0, translation_noise) for v in t]
        yaw = ref.normalize_angle(yaw + rng.normal(0, yaw_noise))
        if kind == 2:
            S = S + rng.normal(0, 2.0, (4, 4))
        if weak in (a, b):
            S = 1e-4 * np.eye(4)
        edges.append((int(a), int(b), t, yaw, S))
    free = 1.0 - np.asarray(constant, np.float64)[:, None]
    start_noise = 1.0 if hard else float(rng.choice((0.0, 0.02, 0.3, 1.0)))
    poses0 = true + free * rng.normal(0, 1, (n, 4)) * start_noise * np.array([1.0, 1.0, 0.1, 1.0])
    wraps = bool(rng.integers(2))
    if wraps:
        poses0[:, 3] += ref.TWO_PI * rng.integers(-2, 3, n)
    nfree = constant.count(0)
    ordering = ORDERINGS[int(rng.integers(3))] if nfree else sref.NATURAL
    given = rng.permutation(nfree) if ordering == sref.GIVEN else None
    if given is not None and cls == "wide":                                # (a random permutation of 300 nodes fills every tile: the reversed
        given = np.roll(np.arange(nfree)[::-1], int(rng.integers(nfree)))   # order, rotated, keeps the restatement's factorisations affordable)
    options = dict(initial_trust_region_radius=float(rng.choice(RADII)), parameter_tolerance=float(rng.choice((3e-3, 1e-6, 1e-2))),
                   function_tolerance=float(rng.choice((1e-6, 1e-8, 1e-3))), max_solver_time_in_seconds=600.0,
                   max_num_iterations=int(rng.integers(0, 4 if cls == "wide" else 13)))
    if hard:                                                               # a wide first radius and tight tolerances: steps get rejected
        options.update(initial_trust_region_radius=1e4, parameter_tolerance=1e-6, function_tolerance=1e-8)
    # covariance pairs: free-free, with a constant node, (a, a), both directions, duplicates -- or none
    pairs = []
    if n >= 2 and rng.random() < 0.9:
        n_pairs = int(rng.choice((1, 3, 9, 20))) if cls == "wide" else int(rng.choice((1, 4, 12, 40)))
        for _ in range(n_pairs):
            a, b = (int(v) for v in (joined[int(rng.integers(len(joined)))] if joined and rng.random() < 0.5 else rng.integers(n, size=2)))
            pairs.append((a, b))
            kind = rng.random()
            if kind < 0.25:
                pairs.append((b, a))
            elif kind < 0.4:
                pairs.append((a, a))
            elif kind < 0.5:
                pairs.append((a, b))
        pairs.append((int(np.flatnonzero(np.asarray(constant))[0]), int(rng.integers(n))))
    # a budget that forces two and more slabs (32 columns each) on some seeds
    max_solve_bytes = 0 if rng.random() < 0.4 else 8 * 4 * max(nfree, 1) * 32 * int(rng.choice((1, 2)))
    sc = SimpleNamespace(seed=seed, size_class=cls, n=n, topology=topology, constant=constant, edges=edges, poses0=poses0, true=true,
                         nfree=nfree, nf=4 * nfree, ordering=ordering, given=given, options=options, cov_pairs=pairs,
                         max_solve_bytes=max_solve_bytes, all_constant=all_constant or nfree == 0, rank_deficient_by_design=rank_deficient,
                         lonely=lonely, weak=weak, wraps=wraps, pairs=[])
    sc.g = dict(n=n, constant=constant, edges=edges, poses0=poses0, pairs=[])
    return sc


def wrapped_yaw_errors(sc):
    """how many edges' yaw errors at the start poses lie a turn or more off before the wrap"""
    if not sc.edges:
        return 0
    return int((np.abs(ref.unwrapped_yaw_errors(sc.g, sc.poses0)) > math.pi).sum())


# ---- registration scenes: over the ring of 12 submaps (tests/pose_graph_ref.ring_graph) -----------------------------
RING = 12


def registration_scene(seed):
    rng = np.random.default_rng([seed, REG_WORD])
    pairs = []
    for _ in range(int(rng.integers(3, 9))):
        a = int(rng.integers(RING))
        b = (a + int(rng.integers(1, 3))) % RING                           # neighbours on the ring: the submaps overlap
        pairs.append((a, b))
        kind = rng.random()
        if kind < 0.25:
            pairs.append((b, a))
        elif kind < 0.4:
            pairs.append((a, b))
    constant = np.zeros(RING, np.int32)
    constant[rng.choice(RING, int(rng.integers(1, 4)), replace=False)] = 1
    a, b = (int(v) for v in np.flatnonzero(constant)[[0, -1]])
    pairs.append((a, (a + 1) % RING))                                      # a pair on a constant node
    g = ref.ring_graph(RING, seed=0)
    edges = [g["edges"][int(k)] for k in rng.choice(len(g["edges"]), int(rng.integers(2, 6)), replace=False)]
    k = int(rng.integers(RING))
    edges.append((k, (k + 5) % RING, rng.normal(0, 0.3, 3), float(rng.normal(0, 0.1)), rng.normal(0, 3, (4, 4))))
    poses0 = g["poses0"] + rng.normal(0, 1, (RING, 4)) * float(rng.choice((0.0, 0.01, 0.05))) * (1.0 - constant[:, None])
    ordering = ORDERINGS[int(rng.integers(3))]
    nfree = int((constant == 0).sum())
    return SimpleNamespace(seed=seed, pairs=pairs, constant=constant.tolist(), edges=edges, poses0=poses0, ordering=ordering,
                           given=rng.permutation(nfree) if ordering == sref.GIVEN else None, max_num_iterations=int(rng.integers(1, 7)),
                           radius=float(rng.choice(RADII)))


def scene(seed):
    return SimpleNamespace(seed=seed, matrix=matrix_scene(seed), graph=graph_scene(seed), registration=registration_scene(seed))


def describe(sc):
    m, g, r = sc.matrix, sc.graph, sc.registration
    bad = ", ".join(f"{v.kind} at row {v.row}" for v in m.bad) or "none"
    return (f"matrix: {m.rows} block rows ({m.size_class}), {m.family}, {len(m.pairs)} pairs, {len(m.l_tiles)} tiles, m {m.m}"
            f"{' in place' if m.in_place else ''}, bad pivot {bad}; graph: {g.n} nodes ({g.size_class}), {g.nfree} free, {g.topology}, "
            f"{len(g.edges)} edges, ordering {g.ordering}, {g.options}, {len(g.cov_pairs)} covariance pairs, budget {g.max_solve_bytes}; "
            f"registration: {len(r.pairs)} constraints, constant {r.constant}, {len(r.edges)} edges, ordering {r.ordering}")
