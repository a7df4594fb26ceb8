"""Scripted-survival inputs for the scan kernels' survivor queues, and a host model of how the Hamming
family deals out work (plain numpy, no GPU).

Every neighbour is its centre's read with mismatches placed at chosen cycles, so a test decides pair by
pair at which cycle the pair dies.  The model (`regimes`) says which of the kernels' decisions an input
drives - it is a COVERAGE check only; the expected result of every test is the CPU oracle.

Convention of a script: `death[t, s]` is the 1-based cycle of the pair's last planted mismatch, 0 = never.
A pair with death d > 0 gets min(k + 1, d) mismatches, the last at cycle d and the others at random
earlier cycles: with d >= k + 1 it dies at cycle d (its (k + 1)-th mismatch), with d <= k it has only d
mismatches and is a duplicate at distance d.  A "never" pair gets 0..k mismatches anywhere.
"""
from __future__ import annotations

import numpy as np

# ---- the kernels' constants, mirrored (file:line of well_duplicates_amd/csrc) -------------------------
K_WAVES = 4                 # wd_shared.h:39         kWaves = kBlock / kWave
K_PASS = 127                # wd_shared.h:45         kPass
K_MAX_PASSES = 4            # wd_shared.h:46         kMaxPasses
K_FINISH_ALL_MAX = 64       # scan_queue.inc:23      kFinishAllMax
K_QCAP = 128                # scan_queue.inc:25      WD_QCAP -> kQCap (:30)
K_FINISH_IN_PLACE = 40      # scan_queue.inc:37      kFinishInPlace
K_LW_TARGETS = 256          # scan_lines.inc:26      kLwTargets (make_line_tables' other cut, line_tables.inc)
K_LW_PAIRS = 12288          # scan_lines.inc:27      kLwPairs
K_LW_STEP = 128             # scan_lines.inc:29      kLwStep = 2 * kWave
K_LW_QCAP = 128             # scan_lines.inc:30      kLwQCap
K_LW_IN_PLACE = 43          # scan_lines.inc:31      kLwInPlace
MAX_ROUND = 8               # scan_queue.inc:262     nb = min(MAXB, nb * 2), MAXB = 8
IN_PLACE_CHUNK = 4          # scan_queue.inc:756, scan_lines.inc:293   j += 4


def finish_from(k: int) -> int:
    return 8 + 4 * max(k, 0)                # device_common.inc:45


def auto_first(k: int) -> int:
    """Cycles of the first round in the plane layout with queue_first = 0 (welldup_queue.hip:42,
    welldup_scan.hip:438); the interleaved layout always reads one dword: 4 (welldup_queue.hip:35)."""
    return 2 if k <= 0 else 3 if k == 1 else 5 if k == 2 else 6 if k == 3 else 8


def first_round(k: int, layout: str) -> int:
    return 4 if layout == "il" else auto_first(k)


def round_starts(B1: int, L: int, layout: str):
    """[(j, nb)] of the drain rounds that exist: q_drain, scan_queue.inc:208-262."""
    j = min(B1, L)
    nb = 4 if (layout == "il" and j % 4 == 0) else 1
    out = []
    while j < L:
        out.append((j, nb))
        j += nb
        nb = min(MAX_ROUND, nb * 2)
    return out


# ---- geometry ------------------------------------------------------------------------------------------
class Geometry:
    """T targets of K slots in `levels` rings, all wells disjoint: target t's centre is well t (K + 1), its
    neighbours the next K wells - so pair order by neighbour well is (target, slot) order."""

    def __init__(self, T: int, K: int, levels: int):
        assert K >= levels >= 1
        self.T, self.K, self.levels = T, K, levels
        self.n = T * (K + 1)
        self.centre = (np.arange(T, dtype=np.int64) * (K + 1)).astype(np.int32)
        self.nbr = (self.centre[:, None] + 1 + np.arange(K, dtype=np.int32)[None, :]).reshape(-1).astype(np.int32)
        cuts = np.linspace(0, K, levels + 1).astype(np.int32)
        assert (np.diff(cuts) > 0).all()
        self.lvl_off = (np.arange(T, dtype=np.int32)[:, None] * K + cuts[None, :]).astype(np.int32)

    def csr(self):
        return self.centre, self.lvl_off, self.nbr


class Script:
    """One tile: planes [L][n] uint8, filt [n] uint8, codes [n, L] (0 = N, 1..4 = ACGT), valid [T] bool,
    death [T, K] as asked for (None for unscripted inputs)."""

    def __init__(self, geom, L, k, codes, planes, filt, death=None):
        self.geom, self.L, self.k = geom, L, k
        self.codes, self.planes, self.filt, self.death = codes, planes, filt, death
        self.valid = (filt[geom.centre] & 1).astype(bool)

    def mismatches(self):
        """bool [T, K, L]: the realised mismatches (codes compared, not the plan)."""
        g = self.geom
        c = self.codes[g.centre]                                  # [T, L]
        w = self.codes[g.nbr].reshape(g.T, g.K, self.L)
        return w != c[:, None, :]

    def death_index(self, k: int):
        """int [T, K]: 0-based cycle of the (k + 1)-th mismatch, L if there is none (a duplicate)."""
        cum = np.cumsum(self.mismatches(), axis=2, dtype=np.int16)
        over = cum > k
        return np.where(over.any(axis=2), over.argmax(axis=2), self.L).astype(np.int32)

    def model_duplicates(self, k: int):
        """bool [T, K]: pairs the Hamming model counts (valid centre, at most k mismatches)."""
        return (self.death_index(k) == self.L) & self.valid[:, None]


def codes_to_bytes(rng, codes):
    """BCL bytes: a no-call is 0, else random non-zero quality bits above the base."""
    q = rng.integers(1, 41, size=codes.shape)
    return np.where(codes == 0, 0, (q << 2) | ((codes - 1) & 3)).astype(np.uint8)


def filter_bytes(rng, n, bad):
    """Bit 0 is the filter; the other bits are noise the kernels must mask."""
    f = ((rng.integers(0, 128, size=n) << 1) | 1).astype(np.uint8)
    f[bad] &= 0xFE
    return f


def random_codes(rng, shape, nocall=0.06):
    c = rng.integers(1, 5, size=shape)
    return np.where(rng.random(shape) < nocall, 0, c).astype(np.int8)


def finish(rng, geom, L, k, codes, bad_centres=(), bad_nbr_frac=0.02, death=None):
    bad = np.zeros(geom.n, dtype=bool)
    bad[geom.centre[np.asarray(bad_centres, dtype=np.int64)]] = True
    nb = rng.random(geom.nbr.shape[0]) < bad_nbr_frac              # neighbours that fail the filter: must not matter
    bad[geom.nbr[nb]] = True
    b = codes_to_bytes(rng, codes)
    planes = [np.ascontiguousarray(b[:, c]) for c in range(L)]
    return Script(geom, L, k, codes, planes, filter_bytes(rng, geom.n, bad), death)


def build(rng, geom: Geometry, L: int, k: int, death, bad_centres=()):
    """The scripted input: see the module docstring for the convention."""
    T, K = geom.T, geom.K
    death = np.asarray(death, dtype=np.int32)
    assert death.shape == (T, K) and death.min() >= 0 and death.max() <= L
    cen = random_codes(rng, (T, L))
    dies = death > 0
    limit = np.where(dies, death - 1, L)                           # planted mismatches besides the last lie before it
    cnt = np.where(dies, np.minimum(k + 1, death) - 1, rng.integers(0, k + 1, size=(T, K)))
    cnt = np.minimum(cnt, limit)
    keys = rng.random((T, K, L))
    idx = np.arange(L)[None, None, :]
    keys[idx >= limit[:, :, None]] = 2.0
    rank = np.argsort(np.argsort(keys, axis=2), axis=2)
    mm = rank < cnt[:, :, None]
    mm |= dies[:, :, None] & (idx == (death - 1)[:, :, None])
    base = np.broadcast_to(cen[:, None, :], (T, K, L)).astype(np.int64)
    sub = (base + rng.integers(1, 5, size=(T, K, L))) % 5          # a different one of the five (N <-> base included)
    nb_codes = np.where(mm, sub, base).astype(np.int8)
    codes = np.zeros((geom.n, L), dtype=np.int8)
    codes[geom.centre] = cen
    codes[geom.nbr] = nb_codes.reshape(T * K, L)
    return finish(rng, geom, L, k, codes, bad_centres, death=death)


def add_edit_scripts(rng, script: Script, every=7):
    """The Levenshtein script kinds, over every `every`-th pair: the centre shifted by one cycle from position p
    on (edit distance <= 2, large Hamming distance), or one insertion and one deletion at different places."""
    g, L = script.geom, script.L
    codes = script.codes.copy()
    for p in range(0, g.T * g.K, every):
        t = p // g.K
        c = codes[g.centre[t]].tolist()
        if (p // every) % 2 == 0:
            at = int(rng.integers(0, L))
            s = c[:at] + [int(rng.integers(0, 5))] + c[at:L - 1]
        else:
            a, b = (int(v) for v in rng.choice(L, size=2, replace=False))
            s = list(c)
            del s[a]
            s.insert(min(b, len(s)), int(rng.integers(0, 5)))
        codes[g.nbr[p]] = s[:L]
    b = codes_to_bytes(rng, codes)
    planes = [np.ascontiguousarray(b[:, c]) for c in range(L)]
    return Script(g, L, script.k, codes, planes, script.filt, None)


def shared_prefix(rng, geom: Geometry, L: int, p: int, bad_centres=()):
    """Every read shares its first p cycles (primer, adaptor) and is random after that."""
    codes = random_codes(rng, (geom.n, L))
    codes[:, :p] = random_codes(rng, (1, p))
    return finish(rng, geom, L, 0, codes, bad_centres)


# ---- how the kernels deal out work ----------------------------------------------------------------------
def deal_queue(valid, K: int, tpb: int):
    """k_scan_q, targets in file order (sort_targets = 0): per block of tpb targets the (valid target, pass)
    items in order (scan_queue.inc:572-583), dealt to the 4 waves round-robin (:606, :658).
    -> [block][wave] -> [(target, first slot, slots)]"""
    T = valid.shape[0]
    out = []
    for t0 in range(0, T, tpb):
        items = []
        for t in range(t0, min(T, t0 + tpb)):
            if valid[t]:
                for s0 in range(0, K, K_PASS):
                    items.append((t, s0, min(K_PASS, K - s0)))
        out.append([items[w::K_WAVES] for w in range(K_WAVES)])
    return out


def deal_lines(T: int, K: int, line_pairs: int):
    """k_scan_lines: the pairs in (target, slot) order cut into blocks of line_pairs (make_line_tables,
    line_tables.inc; its cut at 256 targets must not come first), a wave's steps are windows of 128
    consecutive pairs taken in turn (scan_lines.inc:214).  -> [block][wave] -> [(first pair, pairs)]"""
    P = T * K
    assert line_pairs % (K_WAVES * K_LW_STEP) == 0 and line_pairs // K + 2 <= K_LW_TARGETS
    out = []
    for p0 in range(0, P, line_pairs):
        np_ = min(line_pairs, P - p0)
        wins = [(p0 + w0, min(K_LW_STEP, np_ - w0)) for w0 in range(0, np_, K_LW_STEP)]
        out.append([wins[w::K_WAVES] for w in range(K_WAVES)])
    return out


REGIME_ROWS = ("queued_0", "queued_mid", "queued_top", "inplace_at", "inplace_mid", "inplace_full",
               "push_to_cap", "overflow_drains", "die_round_0", "die_round_1", "die_round_2", "die_round_3",
               "die_round_later", "die_short_last_round", "finish_le64", "finish_eq64", "finish_eq65", "finish_gt64",
               "inplace_chunk_death", "inplace_ragged_chunk_death")


def _drain(R, q, B1, k, L, layout):
    """q_drain (scan_queue.inc:204-265) on the death indices of the queued entries."""
    F = finish_from(k)
    q = np.asarray(q)
    reached = False
    for r, (j, nb) in enumerate(round_starts(B1, L, layout)):
        n = q.shape[0]
        if n == 0:
            break
        if j >= F:
            if not reached:
                reached = True
                R["finish_le64"] += n <= K_FINISH_ALL_MAX
                R["finish_eq64"] += n == K_FINISH_ALL_MAX
                R["finish_eq65"] += n == K_FINISH_ALL_MAX + 1
                R["finish_gt64"] += n > K_FINISH_ALL_MAX
            if n <= K_FINISH_ALL_MAX:
                break                                              # q_finish_all
        nc = min(nb, L - j)
        dead = int(((q >= j) & (q < j + nc)).sum())
        R["die_round_%s" % (r if r < 4 else "later")] += dead
        if nc < nb:
            R["die_short_last_round"] += dead
        q = q[q >= j + nc]


def regimes(script: Script, B1: int, k: int, L: int, tpb: int, layout: str, line_pairs: int = 0):
    """Counts of the decisions the Hamming family takes on this input (REGIME_ROWS).  layout: "plane" or "il";
    line_pairs > 0: the line walk (windows of 128 pairs, thresholds 43 and 128) instead of k_scan_q."""
    assert L == script.L
    g = script.geom
    di = script.death_index(k)
    di = np.where(script.valid[:, None], di, -1)                  # pairs of a filtered centre are never alive
    flat = di.reshape(-1)
    if line_pairs:
        thr, cap = K_LW_IN_PLACE, K_LW_QCAP
        dealt = [[[flat[p:p + m] for p, m in wave] for wave in blk] for blk in deal_lines(g.T, g.K, line_pairs)]
    else:
        thr, cap = K_FINISH_IN_PLACE, K_QCAP
        dealt = [[[di[t, s0:s0 + m] for t, s0, m in wave] for wave in blk] for blk in deal_queue(script.valid, g.K, tpb)]
    R = {r: 0 for r in REGIME_ROWS}
    n1 = min(B1, L)
    n_chunks = (L - B1 + IN_PLACE_CHUNK - 1) // IN_PLACE_CHUNK
    ragged = (L - B1) % IN_PLACE_CHUNK != 0
    for blk in dealt:
        for wave in blk:
            queue, qn = [], 0
            for d in wave:
                alive = d[d >= n1]
                s = alive.shape[0]
                if s == 0:
                    R["queued_0"] += 1
                    continue
                if B1 >= L:
                    continue                                       # the whole read was the first round
                if s >= thr:
                    R["inplace_at"] += s == thr
                    R["inplace_mid"] += thr < s < d.shape[0]
                    R["inplace_full"] += s == d.shape[0]
                    dying = alive[alive < L]
                    chunk = (dying - B1) // IN_PLACE_CHUNK
                    R["inplace_chunk_death"] += int((chunk < n_chunks - (1 if ragged else 0)).sum())
                    R["inplace_ragged_chunk_death"] += int((chunk == n_chunks - 1).sum()) if ragged else 0
                    continue
                R["queued_mid"] += s < thr - 1
                R["queued_top"] += s == thr - 1
                if qn + s > cap:
                    R["overflow_drains"] += 1
                    _drain(R, np.concatenate(queue), B1, k, L, layout)
                    queue, qn = [], 0
                elif qn + s == cap:
                    R["push_to_cap"] += 1
                queue.append(alive)
                qn += s
            if qn:
                _drain(R, np.concatenate(queue), B1, k, L, layout)
    return {r: int(v) for r, v in R.items()}


def possible_rows(B1: int, k: int, L: int, layout: str, units_per_wave: int, thr: int):
    """The rows of REGIME_ROWS an input CAN enter at these parameters - from the code's structure alone: which drain
    rounds exist before the all-at-once finish takes over, whether a last round or chunk is short, whether a wave
    sees enough units to fill its queue."""
    rows = {"queued_0", "queued_mid", "queued_top", "inplace_at", "inplace_mid", "inplace_full"}
    if B1 >= L:
        return {"queued_0"}
    many = units_per_wave * (thr - 1) > K_FINISH_ALL_MAX           # a wave can queue more than 64 entries
    if units_per_wave * (thr - 1) > K_QCAP:
        rows |= {"push_to_cap", "overflow_drains"}
    F = finish_from(k)
    for r, (j, nb) in enumerate(round_starts(B1, L, layout)):
        if j >= F and not many:
            break
        rows.add("die_round_%s" % (r if r < 4 else "later"))
        if L - j < nb:
            rows.add("die_short_last_round")
    if any(j >= F for j, _ in round_starts(B1, L, layout)):
        rows.add("finish_le64")
        if many:
            rows |= {"finish_eq64", "finish_eq65", "finish_gt64"}
    rows.add("inplace_chunk_death") if L - B1 >= IN_PLACE_CHUNK else None
    if (L - B1) % IN_PLACE_CHUNK:
        rows.add("inplace_ragged_chunk_death")
    return rows


# ---- scripts that enter the regimes ----------------------------------------------------------------------
def _deaths_of(rng, kind, n, k, L, B1):
    """Death cycles (1-based, 0 = never) of n first-round survivors: all > B1."""
    F = finish_from(k)
    if kind == "never":
        return np.zeros(n, dtype=np.int32)
    if kind == "early":                                            # in the first drain rounds, before finish_from(k)
        return rng.integers(B1 + 1, B1 + 3, size=n).astype(np.int32)
    if kind == "long":                                             # alive in the last round, whatever its length
        return rng.choice(np.array([0, L], dtype=np.int32), size=n)
    if kind == "late":                                             # alive when the drain reaches finish_from(k)
        return rng.integers(min(F + 9, L - 1), L + 1, size=n).astype(np.int32)
    assert kind == "spread"
    d = rng.integers(B1 + 1, L + 1, size=n).astype(np.int32)
    return np.where(rng.random(n) < 0.25, 0, d)


def scripted_deaths(rng, geom: Geometry, L: int, k: int, B1: int, waves, thr: int, cap: int, striped: bool = False):
    """death [T, K] for the units `waves` deals out ([block][wave] -> units, a unit = (first pair of the flat
    (target, slot) order, pairs)) and a first round of B1 cycles.  Every pair dies inside the first round unless its
    unit's recipe makes it a survivor.  The waves take programs in turn: the in-place threshold from both sides, a
    queue filled to exactly `cap` and then one more, exactly 64 / exactly 65 / more than 64 / a few entries alive at
    finish_from(k), a queue of entries that die all along the drain; then random recipes."""
    T, K = geom.T, geom.K
    assert k + 1 <= B1 and B1 + 2 < min(L, finish_from(k))
    death = rng.integers(k + 1, B1 + 1, size=T * K).astype(np.int32)
    if striped:
        # every third pair in file order survives the first round: any 128 consecutive pairs hold 42 or 43
        surv = np.arange(0, T * K, 3)
        death[surv] = _deaths_of(rng, "spread", surv.shape[0], k, L, B1)
        return death.reshape(T, K)

    def put(unit, s, kinds):
        """s survivors at random slots of the unit; kinds = [(kind, how many), ...], the last kind takes the rest"""
        p0, m = unit
        s = min(s, m)
        slots = p0 + rng.choice(m, size=s, replace=False)
        left = s
        for i, (kind, share) in enumerate(kinds):
            n = left if i == len(kinds) - 1 else min(left, share)
            death[slots[s - left:s - left + n]] = _deaths_of(rng, kind, n, k, L, B1)
            left -= n

    S, full = [("spread", 0)], 1 << 20
    programs = [
        [(thr - 1, S), (thr, S), (thr + 1, S), (full, S), (0, S), (1, S), (90, S), (thr - 1, [("late", 0)]),
         (thr, [("long", 0)]), (20, S), (60, S), (5, [("never", 0)])],
        [(cap // 4, S)] * 4 + [(1, [("never", 0)]), (10, S)],
        [(32, [("never", 0)]), (32, [("never", 0)]), (20, [("early", 0)])],
        [(32, [("never", 0)]), (33, [("never", 0)]), (20, [("early", 0)])],
        [(30, [("long", 22), ("late", 0)])] * 3,
        [(10, [("early", 5), ("never", 0)])],
        [(38, S)] * 3,
    ]
    flat_waves = [w for blk in waves for w in blk]
    for i, wave in enumerate(flat_waves):
        prog = programs[i % len(programs)]
        if len(wave) < len(prog):
            # a wave of a unit or two: one recipe of the first program each, in turn
            for j, unit in enumerate(wave):
                put(unit, *programs[0][(i + j) % len(programs[0])])
            continue
        for unit, (s, kinds) in zip(wave, prog):
            put(unit, s, kinds)
        if i >= len(programs):                                     # (the first round of programs stays exact)
            for unit in wave[len(prog):]:
                put(unit, int(rng.choice([0, 1, 3, 17, 38, 45, 127])), S)
    return death.reshape(T, K)


# ---- the cases both test modules use ---------------------------------------------------------------------
class Case:
    """An input of two tiles with different scripts, built for one kernel (k_scan_q: "queue", units = passes of 127
    slots at 64 targets per block; k_scan_lines: "lines", units = windows of 128 pairs in blocks of 12288), one
    threshold and one layout's first round."""

    def __init__(self, name, kernel, T, K, levels, L, k, layout, kind="scripted", seed=0):
        self.name, self.kernel, self.L, self.k, self.layout, self.kind = name, kernel, L, k, layout, kind
        self.geom = Geometry(T, K, levels)
        self.tpb, self.line_pairs = 64, K_LW_PAIRS
        self.B1 = first_round(k, layout)
        self.mode = 0 if k == 0 else 1
        # centres that fail the filter: only behind the blocks whose waves run the exact programs
        self.bad = [t for t in (T - 70, T - 41, T - 7, T - 6, T - 1) if t >= 0]
        self.tiles = []
        for i in range(2):
            rng = np.random.default_rng([seed, i, T, K, L, k, layout == "il", kernel == "lines"])
            valid = np.ones(T, dtype=bool)
            valid[self.bad] = False
            if kernel == "lines":
                waves = deal_lines(T, K, self.line_pairs)
                thr, cap = K_LW_IN_PLACE, K_LW_QCAP
            else:
                waves = [[[(t * K + s0, m) for t, s0, m in w] for w in blk] for blk in deal_queue(valid, K, self.tpb)]
                thr, cap = K_FINISH_IN_PLACE, K_QCAP
            death = scripted_deaths(rng, self.geom, L, k, self.B1, waves, thr, cap, striped=kind == "striped")
            self.tiles.append(build(rng, self.geom, L, k, death, self.bad))

    @property
    def thr(self):
        return K_LW_IN_PLACE if self.kernel == "lines" else K_FINISH_IN_PLACE

    def units_per_wave(self, line_pairs=None):
        """what a wave of a full block sees"""
        if self.kernel == "lines":
            return (line_pairs or self.line_pairs) // (K_WAVES * K_LW_STEP)
        return self.tpb * ((self.geom.K + K_PASS - 1) // K_PASS) // K_WAVES

    def regimes(self, tile, line_pairs=None):
        lp = (line_pairs or self.line_pairs) if self.kernel == "lines" else 0
        return regimes(self.tiles[tile], self.B1, self.k, self.L, self.tpb, self.layout, line_pairs=lp)


def _case_table():
    t = {}
    for layout in ("plane", "il"):
        for k in (0, 1, 2, 3):
            # K = 127: one pass per target, 16 passes per wave; L = 37 > finish_from(3) + 8 and no multiple of 4
            t["q_k%d_%s_L37" % (k, layout)] = ("queue", 200, 127, 5, 37, k, layout)
            # K = 128: a window of the line walk is a target
            t["lw_k%d_%s_L37" % (k, layout)] = ("lines", 200, 128, 4, 37, k, layout)
        # L = 14 < finish_from(2): a drain never reaches the all-at-once finish, its last round is short
        for k in (0, 2, 3):
            t["q_k%d_%s_L14" % (k, layout)] = ("queue", 200, 127, 5, 14, k, layout)
            t["lw_k%d_%s_L14" % (k, layout)] = ("lines", 200, 128, 4, 14, k, layout)
        t["lw_k1_%s_striped" % layout] = ("lines", 200, 128, 4, 37, 1, layout, "striped")
    # two and three passes per target, the last one ragged
    t["q_k2_plane_K254"] = ("queue", 136, 254, 5, 37, 2, "plane")
    t["q_k1_il_K300"] = ("queue", 136, 300, 5, 37, 1, "il")
    return t


CASES = _case_table()
_built = {}


def case(name) -> Case:
    """Built once per process and shared; nothing changes a case after it is built."""
    if name not in _built:
        _built[name] = Case(name, *CASES[name])
    return _built[name]
