"""Inputs shared by the tests of the pack and stitch kernels (tests/test_stitch_cases_cpu.py, tests/test_gpu_stitch_cases.py): small,
deterministic tracker tables made by hand -- no chain kernel, no GPU -- each the smallest input at which one path of
csrc/mvmc_stitch.hip differs, and their expected messages and tables by oracle/stitch_np.py, computed once and shared (treat
everything returned here as read-only).

People are rigid 18-joint clouds, so the mean joint distance of two of them is the distance of their centres; different people stand
more than a metre apart unless a case says otherwise.  Slots beyond n_tracks hold 7.0 or NaN and a plausible local id, and must be
ignored; slot orders and local ids are permuted per chain.

A case names the branches it is meant to reach (``labels``); measured_labels() derives the same set from the case's data alone, and the
CPU test asks for the two to be equal, for every label to be carried by some case and to be absent from some other."""
import functools

import numpy as np

import stitch_np as sn
from multiview_motion_capture_amd.parallel import chains_cap, shard_range

LABELS = ("clamp-low", "clamp-high", "tables-wider", "tables-narrower", "one-frame-chain", "empty-pack", "scan-per-2", "nodes-over-1024",
          "jump-11-rounds", "swap", "rect", "greedy-wrong", "full-16", "at-threshold", "over-threshold", "tie", "non-finite",
          "ids-over-cap", "mask-high-word", "single-chain-shard", "empty-middle-shard", "trailing-empty-shards", "partial-links",
          "layout-mismatch", "rows-overflow", "chains-over-cap")

SHAPE = np.random.default_rng(20).normal(size=(18, 3)) * 0.15
SHAPE_Q = np.round(SHAPE * 64.0) / 64.0          # multiples of 1/64: sums with multiples of 0.5 are exact in float32
DRIFT = np.array([0.002, 0.001, 0.003])         # metres a frame: everybody walks together


def spot(p):
    """where person p stands: sixteen to a circle of 3.5 m (neighbours 1.37 m apart), further circles above.  No three people are in
    line, so that sending A to B and B to C always costs more than keeping B and sending A to C: the optimum is unique and keeps
    everybody who stays (people in a row would tie)."""
    a = 2.0 * np.pi * (p % 16) / 16.0
    return np.array([3.5 * np.cos(a), 3.5 * np.sin(a), 2.0 * (p // 16)])


def tk(who, lid, at=None, bad=None, nudge=None):
    """One tracklet of a chain: the person behind it (None: nobody in particular), its local id, its centre (default: the person's
    spot), ``bad`` = (joint, coordinate, value) written into every frame, ``nudge`` = (joint, xyz) added to one joint."""
    return dict(who=who, lid=lid, at=spot(who) if at is None else np.asarray(at, float), bad=bad, nudge=nudge)


def _crowd(people, rng):
    """the people in a chain-specific slot order, with permuted local ids"""
    order = rng.permutation(np.asarray(people, dtype=np.int64))
    lids = rng.permutation(len(order))
    return [tk(int(p), int(l)) for p, l in zip(order, lids)]


def _build(chains, L, TT, t_msg=None, id_cap=16, max_dist=0.5, exact=False, n_tracks=None, next_id=None, row_cap="exact",
           void_words=None, worlds=(1,), labels=(), b_cap_extra=0, compare="full", extra_splits=(), truth=True, stitch=True, seed=0,
           half_ulp=False):
    B = len(chains)
    F = B * L
    rng = np.random.default_rng([31, seed, B, L])
    params = np.full((F, TT, 68), 7.0)
    joints = np.zeros((F, TT, 18, 3))
    meta = np.zeros((F, TT, 4), np.int32)
    nt = np.zeros(F, np.int32)
    nid = np.zeros(B, np.int32)
    shape = SHAPE_Q if exact else SHAPE
    for b, ch in enumerate(chains):
        assert len(ch) <= TT
        nid[b] = 1 + max([t["lid"] for t in ch], default=-1)
        for t in range(L):
            f = b * L + t
            nt[f] = len(ch)
            joints[f] = 7.0 if b % 2 == 0 else np.nan
            meta[f] = (0, 2, 1, 1)
            for s, trk in enumerate(ch):
                j = shape + trk["at"] + (0.0 if exact else DRIFT * f)
                if trk["nudge"] is not None:
                    j[trk["nudge"][0]] += trk["nudge"][1]
                if half_ulp:
                    # float64 values that do not survive the cast: exactly half-way between two float32 (ties to even), and just
                    # beside half-way on either side
                    j32 = j.astype(np.float32).astype(np.float64)
                    ulp = np.spacing(np.abs(j32).astype(np.float32)).astype(np.float64)
                    j = j32 + ulp * rng.choice([0.5, -0.5, 0.5000001, 0.4999999, -0.5000001], size=j.shape)
                if trk["bad"] is not None:
                    j[trk["bad"][0], trk["bad"][1]] = trk["bad"][2]
                joints[f, s] = j
                params[f, s] = rng.normal(size=68)
                meta[f, s] = (trk["lid"], 2, t + 1, t + 1)
    if n_tracks is not None:
        nt = np.asarray(n_tracks, np.int32)
        assert nt.shape == (F,)
    if next_id is not None:
        nid = np.asarray(next_id, np.int32)
    return dict(params=params, joints=joints, meta=meta, n_tracks=nt, next_id=nid, chain_len=L, t_msg=TT if t_msg is None else t_msg,
                id_cap=id_cap, max_dist=max_dist, row_cap=row_cap, void_words=void_words, worlds=tuple(worlds), labels=frozenset(labels),
                b_cap_extra=b_cap_extra, compare=compare, extra_splits=tuple(extra_splits), truth=truth, stitch=stitch, chains=chains,
                n_chains=B, t_tables=TT)


def _line(xs, lids=None, who=None):
    """tracklets on the x axis"""
    return [tk(None if who is None else who[i], i if lids is None else lids[i], at=(x, 0.0, 0.0)) for i, x in enumerate(xs)]


def _scan(F):
    """chains of one frame: person 0 always, person 1 in a pattern of varying runs -- one or two tracklets a frame"""
    rng = np.random.default_rng([32, F])
    chains = []
    for b in range(F):
        two = (b * 7 // 5 + b // 11) % 3 != 0
        chains.append(_crowd([0, 1] if two else [0], rng))
    return chains


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng([33, sum(map(ord, name))])
    every = lambda B: tuple(sorted({1, 2, 3, B, B + 2}))       # ... the number of chains, and two trailing empty shards
    # ---- pack: clamps and sizes ----
    if name == "clamps":
        # every table full (8 people); n_tracks says how many slots are live: -3, 0, t_max, t_max + 5 among ordinary frames
        chains = [_crowd(range(8), rng) for _ in range(4)]
        return _build(chains, 2, 8, n_tracks=[-3, 3, 0, 3, 8, 3, 13, 5], worlds=every(4),
                      labels={"clamp-low", "clamp-high", "rect", "partial-links", "empty-pack", "single-chain-shard", "trailing-empty-shards"})
    if name == "wider":
        # tables of 8 slots, a message of 4: a frame with 5 live tracklets is cut to 4
        chains = [_crowd([0, 1, 2], rng), _crowd([0, 1, 2, 3, 4], rng), _crowd([1, 2, 3], rng), _crowd([1, 3], rng)]
        return _build(chains, 3, 8, t_msg=4, worlds=every(4),
                      labels={"tables-wider", "clamp-high", "rect", "swap", "empty-pack", "single-chain-shard", "trailing-empty-shards",
                              "partial-links"})
    if name == "narrower":
        # tables of 8 slots, a message of 16, room for two chains more than the shard has
        chains = [_crowd([0, 1, 2, 3], rng), _crowd([0, 1, 2, 3], rng), _crowd([0, 2, 3, 5], rng)]
        return _build(chains, 2, 8, t_msg=16, b_cap_extra=2, worlds=every(3), void_words=np.zeros(3, np.int32),
                      labels={"tables-narrower", "empty-pack", "single-chain-shard", "trailing-empty-shards"})
    if name == "one-frame":
        # chain_len 1: both bound tables of a chain come from the same frame; 32 void words with bits 0, 17 and 31 set
        vw = np.zeros(32, np.int32)
        vw[[0, 17, 31]] = (1, -5, 9)
        chains = [_crowd(p, rng) for p in ([0, 1, 2], [0, 1, 2], [0, 2], [0, 1, 2], [1, 2])]
        return _build(chains, 1, 4, void_words=vw, worlds=every(5),
                      labels={"one-frame-chain", "rect", "swap", "empty-pack", "single-chain-shard", "trailing-empty-shards",
                              "partial-links"})
    if name == "one-chain":
        return _build([_crowd([0, 1, 2], rng)], 3, 8, worlds=(1, 3), labels={"empty-pack", "single-chain-shard", "trailing-empty-shards"})
    if name in ("no-frames-b0", "no-frames-b3"):
        # n_frames 0: the header and an empty local section only.  (With room for no chain at all there is no table to stitch into.)
        b3 = name.endswith("b3")
        return _build([], 2, 8, b_cap_extra=3 if b3 else 0, row_cap=5, stitch=b3, labels={"empty-pack"})
    if name in ("rows-0", "rows-minus-1"):
        chains = [_crowd([0, 1, 2], rng) for _ in range(3)]
        return _build(chains, 2, 4, row_cap=0 if name == "rows-0" else "minus1", worlds=(1, 2), compare="flags", labels={"rows-overflow", "single-chain-shard"})
    # ---- pack: scans ----
    if name.startswith("scan-"):
        F = int(name[5:])
        return _build(_scan(F), 1, 4, worlds=(1, 3),
                      labels={"one-frame-chain", "nodes-over-1024", "rect", "swap"} | ({"scan-per-2"} if F > 1024 else set())
                      | ({"jump-11-rounds"} if F > 1025 else set()))
    if name == "long-links":
        # person 0 in all of 1030 chains of one frame: 1029 links in a row, 11 rounds of pointer jumping; person 1 in every third
        # chain: roots without a successor in between
        chains = [_crowd([0, 1] if b % 3 == 0 else [0], rng) for b in range(1030)]
        return _build(chains, 1, 4, worlds=(1, 2), labels={"one-frame-chain", "nodes-over-1024", "scan-per-2", "jump-11-rounds", "rect", "swap"})
    if name == "rounding":
        chains = [_crowd([0, 1, 2], rng) for _ in range(3)]
        return _build(chains, 2, 4, half_ulp=True, worlds=every(3), labels={"empty-pack", "single-chain-shard", "trailing-empty-shards"})
    # ---- the assignment ----
    if name == "greedy-wrong":
        # nearest first takes 0.40 | 0.36 (0.04), which leaves 0.00 | 0.64 beyond max_dist: two pairs, total 0.70; the optimum keeps the
        # order, three pairs, total 0.62 -- 0.08 below the second best
        return _build([_line([0.0, 0.4, 3.0], [2, 0, 1]), _line([0.64, 3.02, 0.36], [1, 2, 0])], 2, 4, exact=True, truth=False, worlds=(1, 2),
                      labels={"greedy-wrong", "single-chain-shard"})
    if name == "rect-2v5":
        chains = [_crowd([1, 3], rng), _crowd([0, 1, 2, 3, 4], rng)]
        return _build(chains, 2, 8, worlds=(1, 2), labels={"rect", "single-chain-shard", "partial-links"})
    if name == "swap-5v2":
        chains = [_crowd([0, 1, 2, 3, 4], rng), _crowd([3, 1], rng)]
        return _build(chains, 2, 8, worlds=(1, 2), labels={"swap", "single-chain-shard"})
    if name == "full-16":
        chains = [_crowd(range(16), rng) for _ in range(3)]
        return _build(chains, 1, 16, worlds=every(3),
                      labels={"full-16", "one-frame-chain", "empty-pack", "single-chain-shard", "trailing-empty-shards"})
    if name == "nobody":
        chains = [_crowd([0, 1], rng), [], _crowd([0, 1], rng), _crowd([0, 1], rng)]
        return _build(chains, 2, 4, worlds=every(4), labels={"empty-pack", "single-chain-shard", "trailing-empty-shards"})
    if name == "all-far":
        # everybody has moved by a metre between the chains: an assignment exists, no pair survives max_dist
        a = _crowd([0, 1, 2], rng)
        b = [tk(t["who"] + 100, t["lid"], at=t["at"] + (0.0, 0.0, 1.0)) for t in _crowd([0, 1, 2], rng)]
        return _build([a, b], 2, 4, worlds=(1, 2), labels={"single-chain-shard"})
    # ---- at the threshold: every step of the first pair's cost is exact in float32 and in float64 (differences 0.5, squares 0.25,
    # roots 0.5, their sum 9, the quotient 0.5): a match.  The second pair has one joint 1e-3 m further: mean 0.5 + 5.6e-5, no match.
    if name == "threshold":
        a = [tk("a", 1, at=(0.0, 0.0, 0.0)), tk("b", 0, at=(4.0, 0.0, 0.0))]
        b = [tk("b", 0, at=(4.5, 0.0, 0.0), nudge=(7, (1e-3, 0.0, 0.0))), tk("a", 1, at=(0.5, 0.0, 0.0))]
        return _build([a, b], 1, 4, exact=True, truth=False, worlds=(1, 2),
                      labels={"at-threshold", "over-threshold", "one-frame-chain", "single-chain-shard"})
    if name == "tie":
        # two identical tracklets on the previous side: either may take the one person who continues
        a = [tk(0, 2), tk(1, 0), tk(0, 1)]
        b = [tk(1, 1), tk(0, 0)]
        return _build([a, b], 2, 4, compare="tie", truth=False, worlds=(1, 2), labels={"tie", "swap", "single-chain-shard"})
    # ---- non-finite joints: the broken tracklet is live, matches nobody, starts a new identity; the healthy ones are matched ----
    if name == "nan-2x2":
        # costs [[1.43, -], [0.11, -]]: a sentinel of 1e30 in the second column makes both assignments cost 1e30 exactly
        a = [tk("p", 0, at=(0.0, 0.0, 0.0)), tk("q", 1, at=(1.54, 0.0, 0.0))]
        b = [tk("q", 1, at=(1.43, 0.0, 0.0)), tk("r", 0, at=(5.0, 0.0, 0.0), bad=(4, 1, np.nan))]
        return _build([a, b], 2, 4, exact=True, worlds=(1, 2), labels={"non-finite", "swap", "single-chain-shard"})
    if name == "inf-3x3-prev":
        a = [tk("p", 2, at=(0.0, 0.0, 0.0)), tk("x", 0, at=(7.0, 0.0, 0.0), bad=(17, 2, np.inf)), tk("q", 1, at=(1.54, 0.0, 0.0))]
        b = [tk("q", 0, at=(1.43, 0.0, 0.0)), tk("s", 2, at=(9.0, 2.0, 0.0)), tk("p", 1, at=(0.3, 0.0, 0.0))]
        return _build([a, b], 2, 4, exact=True, worlds=(1, 2), labels={"non-finite", "rect", "partial-links", "single-chain-shard"})
    if name == "nan-inf-both":
        a = [tk("x", 0, at=(7.0, 0.0, 0.0), bad=(0, 0, np.nan)), tk("p", 1, at=(0.0, 0.0, 0.0)), tk("q", 2, at=(1.54, 0.0, 0.0))]
        b = [tk("q", 2, at=(1.43, 0.0, 0.0)), tk("y", 1, at=(7.0, 0.0, 0.0), bad=(9, 2, -np.inf)), tk("p", 0, at=(0.45, 0.0, 0.0))]
        c = [tk("p", 0, at=(0.5, 0.0, 0.0)), tk("q", 1, at=(1.4, 0.0, 0.0)), tk("y", 2, at=(7.0, 0.0, 0.0))]
        return _build([a, b, c], 2, 4, exact=True, worlds=(1, 2, 3), labels={"non-finite", "rect", "partial-links", "single-chain-shard"})
    # ---- identity capacity ----
    if name == "id-cap-1":
        chains = [[tk(0, 0)], [tk(0, 0)], [tk(1, 0)], [tk(1, 0)]]
        return _build(chains, 2, 4, id_cap=1, worlds=every(4), labels={"empty-pack", "single-chain-shard", "trailing-empty-shards"})
    if name == "ids-over-cap":
        # the middle chain has handed out 17 identities; its live tracklet of local id 16 is matched on both sides and linked on neither
        chains = [[tk(0, 1), tk(1, 0), tk(2, 2)], [tk(1, 16), tk(0, 3), tk(2, 9)], [tk(2, 0), tk(1, 1), tk(0, 2)]]
        return _build(chains, 2, 8, worlds=every(3),
                      labels={"ids-over-cap", "empty-pack", "single-chain-shard", "trailing-empty-shards", "partial-links"})
    if name == "mask-high":
        # id_cap 64; every chain has handed out 40 identities; ten are live at its ends, local ids 33 .. 39 among them, and eight of the
        # ten continue across every boundary
        chains = []
        for b in range(4):
            people = [p for p in range(12) if p not in ((b % 3), 11 - (b % 2))][:10]
            lids = rng.permutation([33, 34, 35, 36, 37, 38, 39, 0, 5, 20])
            chains.append([tk(int(p), int(l)) for p, l in zip(rng.permutation(people), lids)])
        return _build(chains, 2, 16, id_cap=64, next_id=[40] * 4, worlds=(1, 2, 4),
                      labels={"mask-high-word", "single-chain-shard", "partial-links"})
    # ---- shards ----
    if name == "walk-3":
        # one person walks through three chains -- at world 3 three shards of one chain each: the resolve chains through `resolved`
        chains = [[tk(0, 0)], [tk(5, 0), tk(0, 1)], [tk(0, 0)]]
        return _build(chains, 2, 4, worlds=every(3),
                      labels={"rect", "swap", "empty-pack", "single-chain-shard", "trailing-empty-shards"})
    if name == "partial-links":
        # the third chain has five identities; only its local ids 1 and 3 continue someone: the others are numbered around them
        chains = [[tk(0, 0), tk(1, 1)], [tk(1, 0), tk(0, 1)], [tk(7, 0), tk(0, 1), tk(8, 2), tk(1, 3), tk(9, 4)],
                  [tk(9, 0), tk(8, 1), tk(0, 2)]]
        return _build(chains, 1, 8, worlds=every(4),
                      labels={"partial-links", "one-frame-chain", "rect", "swap", "empty-pack", "single-chain-shard", "trailing-empty-shards"})
    if name == "empty-middle":
        # [A, a pack of zero frames, B]: shard_range never makes this, the kernel claims to skip it
        chains = [_crowd([0, 1, 2], rng), _crowd([0, 1, 2], rng), _crowd([0, 2, 3], rng), _crowd([0, 2, 3], rng)]
        return _build(chains, 2, 4, worlds=(1,), extra_splits=(dict(name="a-0-b", ranges=((0, 2), (2, 2), (2, 4)), b_cap=2),),
                      labels={"empty-middle-shard", "empty-pack"})
    # ---- flags: only info[2] is compared (restatement and kernel treat a void shard's chains differently) ----
    if name == "flags":
        chains = [_crowd([0, 1, 2], rng) for _ in range(4)]
        return _build(chains, 2, 4, worlds=(1,), labels={"layout-mismatch", "chains-over-cap"},
                      extra_splits=(dict(name="t-max-differs", ranges=((0, 2), (2, 4)), b_cap=2, patches=((1, 2, 8),), compare="flags"),
                                    dict(name="chains-over-cap", ranges=((0, 2), (2, 4)), b_cap=2, patches=((0, 0, 3),), compare="flags")))
    raise KeyError(name)


NAMES = ("clamps", "wider", "narrower", "one-frame", "one-chain", "no-frames-b0", "no-frames-b3", "rows-0", "rows-minus-1",
         "scan-1023", "scan-1024", "scan-1025", "scan-2050", "long-links", "rounding", "greedy-wrong", "rect-2v5", "swap-5v2", "full-16",
         "nobody", "all-far", "threshold", "tie", "nan-2x2", "inf-3x3-prev", "nan-inf-both", "id-cap-1", "ids-over-cap", "mask-high",
         "walk-3", "partial-links", "empty-middle", "flags")


# ------------------------------------------------------------------------------------------------------------------------------------
# splits: how a case's chains go to the shards
# ------------------------------------------------------------------------------------------------------------------------------------
def _live(c):
    return np.clip(c["n_tracks"], 0, min(c["t_msg"], c["t_tables"]))


def split_of(c, split):
    """-> dict(ranges [(lo, hi) chains of every shard], b_cap, row_cap, patches ((shard, word, value), ...), compare).  ``split`` is a
    world size (parallel.shard_range) or the name of one of the case's hand-made splits."""
    B, L = c["n_chains"], c["chain_len"]
    if isinstance(split, int):
        sp = dict(ranges=tuple(shard_range(B, r, split) for r in range(split)), b_cap=chains_cap(B, split), patches=(), compare=c["compare"])
    else:
        e = {s["name"]: s for s in c["extra_splits"]}[split]
        sp = dict(ranges=e["ranges"], b_cap=e["b_cap"], patches=e.get("patches", ()), compare=e.get("compare", c["compare"]))
    sp["b_cap"] += c["b_cap_extra"]
    wanted = max(int(_live(c)[lo * L:hi * L].sum()) for lo, hi in sp["ranges"])
    sp["row_cap"] = wanted if c["row_cap"] == "exact" else (wanted - 1 if c["row_cap"] == "minus1" else int(c["row_cap"]))
    return sp


def splits(c):
    return tuple(c["worlds"]) + tuple(s["name"] for s in c["extra_splits"])


PARAMS = tuple((n, s) for n in NAMES for s in splits(case(n)))


def shard_tables(c, lo, hi):
    """the tables of chains [lo, hi)"""
    L = c["chain_len"]
    out = {k: np.ascontiguousarray(c[k][lo * L:hi * L]) for k in ("params", "joints", "meta", "n_tracks")}
    out["next_id"] = np.ascontiguousarray(c["next_id"][lo:hi])
    return out


@functools.lru_cache(maxsize=None)
def reference(name, split):
    """-> dict(split fields, messages (shards, words) int32 by sn.pack_np with the split's patches applied, stitched = sn.stitch_np of
    them, or None where the case has no stitch)."""
    c = case(name)
    sp = split_of(c, split)
    msgs = []
    for lo, hi in sp["ranges"]:
        t = shard_tables(c, lo, hi)
        msgs.append(sn.pack_np(t["params"], t["joints"], t["meta"], t["n_tracks"], t["next_id"], c["chain_len"], sp["b_cap"], sp["row_cap"],
                               t_msg=c["t_msg"], void_words=c["void_words"], max_dist=c["max_dist"], id_cap=c["id_cap"]))
    msgs = np.stack(msgs)
    for r, w, v in sp["patches"]:
        msgs[r, w] = v
    st = sn.stitch_np(msgs, sp["b_cap"], c["t_msg"], sp["row_cap"], c["max_dist"], c["id_cap"]) if c["stitch"] else None
    return dict(sp, messages=msgs, stitched=st)


# ------------------------------------------------------------------------------------------------------------------------------------
# the case's data, read without the restatement: boundary tables, expected pairs, the labels it really carries
# ------------------------------------------------------------------------------------------------------------------------------------
def bound_tables(c):
    """-> ids (B,2,T) i32 (-1 = not live), joints (B,2,T,18,3) f32 (NaN where not live): first / last frame of every chain"""
    B, L, T = c["n_chains"], c["chain_len"], c["t_msg"]
    ids = -np.ones((B, 2, T), np.int32)
    jo = np.full((B, 2, T, 18, 3), np.nan, np.float32)
    nt = _live(c)
    for b in range(B):
        for side, f in ((0, b * L), (1, b * L + L - 1)):
            ids[b, side, :nt[f]] = c["meta"][f, :nt[f], 0]
            jo[b, side, :nt[f]] = c["joints"][f, :nt[f]].astype(np.float32)
    return ids, jo


def boundaries(c):
    """-> list of (g, live slots of chain g - 1's last frame, their joints, live slots of chain g's first frame, their joints)"""
    ids, jo = bound_tables(c)
    out = []
    for g in range(1, c["n_chains"]):
        ip, inn = np.nonzero(ids[g - 1, 1] >= 0)[0], np.nonzero(ids[g, 0] >= 0)[0]
        out.append((g, ip, jo[g - 1, 1][ip], inn, jo[g, 0][inn]))
    return out


def expected_pairs(c):
    """For a case with ``truth``: {g: sorted [(slot of chain g - 1's last frame, slot of chain g's first frame)]} of the tracklets of one
    person that are live and finite on both sides -- who must be matched, whoever else is broken."""
    nt, L = _live(c), c["chain_len"]
    out = {}
    for g in range(1, c["n_chains"]):
        fp, fn = g * L - 1, g * L
        pairs = []
        for sp_, a in enumerate(c["chains"][g - 1][:nt[fp]]):
            for sn_, b in enumerate(c["chains"][g][:nt[fn]]):
                if a["who"] == b["who"] and a["who"] is not None and np.isfinite(c["joints"][fp, sp_]).all() and np.isfinite(c["joints"][fn, sn_]).all():
                    pairs.append((sp_, sn_))
        out[g] = sorted(pairs)
    return out


def greedy_pairs(cost, max_dist):
    """nearest first: the pairing an optimal assignment must beat"""
    cost = cost.copy()
    pairs = []
    while cost.size and np.isfinite(cost).any():
        i, j = np.unravel_index(np.argmin(cost), cost.shape)
        if cost[i, j] <= max_dist:
            pairs.append((int(i), int(j)))
        cost[i, :] = np.inf
        cost[:, j] = np.inf
    return sorted(pairs)


def measured_labels(c):
    """The labels the case's DATA carries, each by its own definition (nothing here reads c["labels"])."""
    B, L, T, TT, IC = c["n_chains"], c["chain_len"], c["t_msg"], c["t_tables"], c["id_cap"]
    F = B * L
    got = set()
    if (c["n_tracks"] < 0).any(): got.add("clamp-low")
    if (c["n_tracks"] > min(T, TT)).any(): got.add("clamp-high")
    if TT > T: got.add("tables-wider")
    if TT < T: got.add("tables-narrower")
    if L == 1 and F > 0: got.add("one-frame-chain")
    if F > 1024: got.add("scan-per-2")                     # row_offsets_kernel: more than one frame a thread
    if B * IC > 1024: got.add("nodes-over-1024")           # local_ids_kernel: more than one node a thread
    if (c["next_id"] > IC).any(): got.add("ids-over-cap")
    ids, jo = bound_tables(c)
    for g, ip, pj, inn, nj in boundaries(c):
        fp, fn = sn.finite_tracklets(pj), sn.finite_tracklets(nj)
        if len(fp) < len(ip) or len(fn) < len(inn): got.add("non-finite")
        for side in (pj, nj):
            if any(np.array_equal(side[i].view(np.int32), side[j].view(np.int32)) for i in range(len(side)) for j in range(i)): got.add("tie")
        if len(fp) == 0 or len(fn) == 0:
            continue
        if len(fp) > len(fn): got.add("swap")
        if len(fp) < len(fn): got.add("rect")
        if len(fp) == 16 == len(fn): got.add("full-16")
        cost = sn.boundary_costs(pj[fp], nj[fn])
        if max(len(fp), len(fn)) <= 7:
            total, pairs = sn.match_boundary_brute(pj, nj, c["max_dist"])
            assigned = sn.match_boundary_brute(pj, nj, np.inf)[1]
            d = [cost[list(fp).index(i), list(fn).index(j)] for i, j in assigned]
            if any(x == c["max_dist"] for x in d): got.add("at-threshold")
            if any(c["max_dist"] < x <= c["max_dist"] + 0.01 for x in d): got.add("over-threshold")
            if [(int(fp[i]), int(fn[j])) for i, j in greedy_pairs(cost, c["max_dist"])] != pairs: got.add("greedy-wrong")
    # what depends on the sharding
    one = reference_ids(c)
    if one is not None and len(one) and np.bincount(one[one >= 0]).max() > 1025: got.add("jump-11-rounds")   # > 2^10 links in a row
    for s in splits(c):
        sp = split_of(c, s)
        sizes = [hi - lo for lo, hi in sp["ranges"]]
        if 0 in sizes: got.add("empty-pack")
        if isinstance(s, int) and B > 0 and s > B: got.add("trailing-empty-shards")
        if any(n == 0 and any(sizes[:i]) and any(sizes[i + 1:]) for i, n in enumerate(sizes)): got.add("empty-middle-shard")
        if len(sizes) > 1 and 1 in sizes: got.add("single-chain-shard")
        live = _live(c)
        if any(int(live[lo * L:hi * L].sum()) > sp["row_cap"] for lo, hi in sp["ranges"]): got.add("rows-overflow")
        for r, w, v in sp["patches"]:
            if w == 2 and v != T: got.add("layout-mismatch")
            if w == 0 and v > sp["b_cap"]: got.add("chains-over-cap")
        # the shard boundaries: which local ids of a shard's first chain continue someone
        for lo, hi in sp["ranges"][1:]:
            if lo == 0 or lo >= B or hi == lo:
                continue
            _, ip, pj, inn, nj = boundaries(c)[lo - 1]
            linked = set()
            for i, j in sn.match_boundary_brute(pj, nj, c["max_dist"])[1] if max(len(ip), len(inn)) <= 7 else sn.match_boundary(pj, nj, c["max_dist"]):
                lp, ln_ = int(ids[lo - 1, 1, ip[i]]), int(ids[lo, 0, inn[j]])
                if lp < IC and ln_ < IC:
                    linked.add(ln_)
            if any(l >= 32 for l in linked): got.add("mask-high-word")
            n_first = min(int(c["next_id"][lo]), IC)
            if any(k not in linked and any(l < k for l in linked) for k in range(n_first)): got.add("partial-links")
    return frozenset(got)


def reference_ids(c):
    """gid (B, id_cap) of the single pass over all chains (world 1), or None for a case without a stitch"""
    if not c["stitch"] or c["n_chains"] == 0:
        return None
    name = next(n for n in NAMES if case(n) is c)
    return reference(name, 1)["stitched"]["gid"][:c["n_chains"]]
