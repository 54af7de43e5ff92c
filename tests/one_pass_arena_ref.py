"""The overflow arena of one-pass binning, restated, and frames whose parts hold chosen numbers of points (TEST INFRASTRUCTURE,
numpy only: no GPU, no library).

WHAT IS RESTATED (csrc/pwpp_capi.cpp: build_capacity_table, finish_pending; csrc/pwpp_kernels.hip: k_czm_bin_scatter, k_czm_scan):
`capacity_table` -- the segment of every part, the arena and its room for spilled records, from the observed per-part maxima;
`next_table` -- which table the following batch meets; `parts_of_points` -- the part a point is binned into; `outcome` -- what
becomes of a frame with given part counts under a table: it fits, its overgrown parts are moved inside the arena, or it goes back to
the host, with the FIRST reason in the order the kernel tests them; `predict` -- what arena_stats / redo_stats / one_pass_stats
gain from a batch, the host's choice between a redo in place and a redo of the whole batch included.

THE CASES: a sizing batch of identical frames sets the observed maxima exactly (a cold handle histograms every frame of a batch of
at most 256), then a test batch in which chosen frames carry chosen counts: one limit at its edge, the others well inside.  The counts
follow from the table the test batch meets, which depends on the largest frame of that batch: `Case.built` iterates to the fixed point.
Frames that go back to the host stand in a batch of their own (a redo of the whole batch forgets which other frames had moved parts).
"""
import math

import numpy as np

import list_order_ref as lo

SLOT_ALIGN = 32       # PWPP_SLOT_ALIGN
MAX_RELOC = 64        # PWPP_MAX_RELOC
FEW_FRAMES = 16       # batches of at most so many frames get generous segments and no arena
HI_SPLIT = 0.6        # option hi_split: metres above -sensor_height where the high part begins
SPLIT_ZONES = 1       # option hi_split_zones: the bins of the first zone are stored in two parts
NO_ARENA_FLAG = 2048  # debug_flags: today's segments without an arena


def align(v):
    return (int(v) + SLOT_ALIGN - 1) & ~(SLOT_ALIGN - 1)


# ---------------------------------------------------------------------------------------------------------------
# parts
# ---------------------------------------------------------------------------------------------------------------
def bin_bases(p):
    out = [0]
    for z in range(4):
        out.append(out[-1] + p.num_rings_each_zone[z] * p.num_sectors_each_zone[z])
    return out


def num_bins(p):
    return bin_bases(p)[4]


def split_end(p):
    return bin_bases(p)[SPLIT_ZONES]


def num_parts(p):
    return 2 * num_bins(p) + 2


def bin_of(p, zone, ring, sector):
    return bin_bases(p)[zone] + ring * p.num_sectors_each_zone[zone] + sector


def part_index(p, spec):
    """A part by name: ("lo" | "hi" | "bin", zone, ring, sector), ("rnr",) or ("far",).  "bin": the single part of an unsplit bin."""
    B = num_bins(p)
    if spec[0] == "rnr":
        return 2 * B
    if spec[0] == "far":
        return 2 * B + 1
    b = bin_of(p, *spec[1:])
    assert (spec[0] == "bin") == (b >= split_end(p)), spec
    return 2 * b + (1 if spec[0] == "hi" else 0)


def part_kind(p, part):
    B = num_bins(p)
    if part >= 2 * B:
        return "rnr" if part == 2 * B else "far"
    if part // 2 < split_end(p):
        return "high" if part & 1 else "low"
    bases = bin_bases(p)
    return "zone%d" % max(z for z in range(4) if part // 2 >= bases[z])


def part_name(p, part):
    B = num_bins(p)
    if part >= 2 * B:
        return "rnr" if part == 2 * B else "far"
    return "%d%s" % (part // 2, ("h" if part & 1 else "l") if part // 2 < split_end(p) else "")


def parts_of_points(p, pts):
    """The part every point of a (n, 4) cloud is binned into, for points away from every bin limit (czm_code and part_of: RNR hit,
    out of range, else zone / ring / sector and -- below split_end -- the side of the split height)."""
    x, y, z, w = (pts[:, k].astype(np.float64) for k in range(4))
    B = num_bins(p)
    h = float(p.sensor_height)
    r32 = np.sqrt((pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]).astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        angle = np.degrees(np.arctan2(z, r32))
    rnr = (p.enable_RNR != 0) & (z < -h - 0.8) & (w < p.RNR_intensity_thr) & (angle < p.RNR_ver_angle_thr)
    r = np.hypot(x, y)
    theta = np.arctan2(y, x)
    theta = np.where(theta < 0, theta + 2 * math.pi, theta)
    inside = (r <= p.max_range) & (r > p.min_range)
    mn, mx = p.min_range, p.max_range
    starts = [mn, (7 * mn + mx) / 8.0, (3 * mn + mx) / 4.0, (mn + mx) / 2.0, mx]
    bases = bin_bases(p)
    code = np.full(len(pts), B + 1, np.int64)
    for zone in range(4):
        rings, sectors = p.num_rings_each_zone[zone], p.num_sectors_each_zone[zone]
        here = inside & (r >= starts[zone]) & ((r < starts[zone + 1]) | (zone == 3))
        ring = np.minimum(((r - starts[zone]) / ((starts[zone + 1] - starts[zone]) / rings)).astype(np.int64), rings - 1)
        sector = np.minimum((theta / (2 * math.pi / sectors)).astype(np.int64), sectors - 1)
        code = np.where(here, bases[zone] + ring * sectors + sector, code)
    code = np.where(rnr, B, code)
    zs = np.float32(-h + HI_SPLIT)
    high = ~(pts[:, 2] < zs)
    return np.where(code < split_end(p), 2 * code + high, np.where(code < B, 2 * code, code + B))


# ---------------------------------------------------------------------------------------------------------------
# the capacity table
# ---------------------------------------------------------------------------------------------------------------
class Table:
    """cap[part], arena_base (= the segments together), arena_slots, arena_spill, slots_per_frame, few, cap_max_n"""

    def key(self):
        return (tuple(self.cap), self.arena_slots, self.arena_spill, self.slots_per_frame, self.few, self.cap_max_n)


def capacity_table(observed, max_n, frames, one_pass_scale, split_end, num_bins, debug_flags=0):
    """build_capacity_table: `max_n` as the caller passes it (largest frame + an eighth)."""
    NP = 2 * num_bins + 2
    assert len(observed) == NP
    t = Table()
    t.few = frames <= FEW_FRAMES and one_pass_scale >= 1.0
    scale = (3.75 if t.few else 1.0625) * one_pass_scale / 4.0
    t.cap = []
    for b in range(NP):
        seen = float(observed[b])
        cap = scale * seen + ((2048.0 if t.few else 2.0 * math.sqrt(seen) + 16.0) if one_pass_scale >= 1.0 else 16.0)
        if cap > float(max_n) + 16.0:
            cap = float(max_n) + 16.0
        c = align(int(cap))
        if b < 2 * num_bins and (b & 1) and b // 2 >= split_end:
            c = 0  # the high part of a bin that is not split
        t.cap.append(c)
    run = sum(t.cap)
    arena = 0
    if not t.few and not (debug_flags & NO_ARENA_FLAG):
        biggest = int(max(observed))
        arena = biggest + biggest // 4 + max_n // 16 + 4096
        if one_pass_scale < 1.0:
            arena = int(float(arena) * one_pass_scale)
        arena = align(arena)
        if run + arena >= 1 << 31:
            arena = 0
    t.arena_base = run
    t.arena_slots = arena
    t.arena_spill = arena // 4 if arena // 4 > 2048 else (arena if arena < 2048 else 2048)
    t.slots_per_frame = run + arena
    t.cap_max_n = max_n
    return t


def passed_max_n(largest_frame):
    return largest_frame + largest_frame // 8


def next_table(table, stale, largest_frame, frames, one_pass_scale):
    """(rebuild, probe again): what estimate_batch decides for a batch whose largest frame has `largest_frame` points, given the
    current table (None: a cold handle) and whether finish_pending marked it stale."""
    if table is None:
        return True, True
    again = 2 * largest_frame < table.cap_max_n  # a much smaller sensor: the observed maxima start over
    few = frames <= FEW_FRAMES and one_pass_scale >= 1.0
    return (stale or again or largest_frame > table.cap_max_n or table.few != few), again


# ---------------------------------------------------------------------------------------------------------------
# what becomes of a frame, and of a batch
# ---------------------------------------------------------------------------------------------------------------
class Outcome:
    def __init__(self, kind, reason=None, nov=0, spilled=0, run=0, moved=()):
        self.kind, self.reason, self.nov, self.spilled, self.run, self.moved = kind, reason, nov, spilled, run, tuple(moved)

    def __str__(self):
        return self.kind if self.reason is None else "%s: %s" % (self.kind, self.reason)


def outcome(counts, t):
    over = [b for b in range(len(t.cap)) if counts[b] > t.cap[b]]           # k_czm_scan: c > cap
    if not over:
        return Outcome("fits")
    spilled = int(sum(counts[b] - t.cap[b] for b in over))                  # k_czm_bin_scatter: the points with r >= cap
    nov = len(over)
    run = align(spilled) + sum(align(counts[b]) for b in over)              # moved parts in part order behind the records
    if t.arena_slots == 0:
        return Outcome("host", "no-arena", nov, spilled, 0)
    if nov > MAX_RELOC:
        return Outcome("host", "too-many-parts", nov, spilled, run)
    if spilled > t.arena_spill:                                             # (the binning kernel lost a record: a >= arena_spill)
        return Outcome("host", "spill-full", nov, spilled, run)
    if run > t.arena_slots:
        return Outcome("host", "arena-full", nov, spilled, run)
    return Outcome("moved", None, nov, spilled, run, over)


class Prediction:
    """what a batch adds to arena_stats()[0], redo_stats() and one_pass_stats(); `redo`: None, "in-place" or "whole-batch" """

    def __str__(self):
        return "arena+%d redo+(%d,%d) one-pass+(%d,%d)%s" % ((self.arena,) + self.redo_stats + self.one_pass_stats + (" " + self.redo if self.redo else "",))


def predict(outcomes, sizes, t, num_parts, redo_whole_batch=False):
    F = len(outcomes)
    redo = [f for f, o in enumerate(outcomes) if o.kind == "host"]
    moved = sum(o.kind == "moved" for o in outcomes)
    pr = Prediction()
    pr.redo = None
    if not redo:
        pr.arena, pr.redo_stats, pr.one_pass_stats = moved, (F, 0), (1, 0)
        return pr
    in_place = not redo_whole_batch
    runs = sum(1 for i, f in enumerate(redo) if i == 0 or f != redo[i - 1] + 1)
    if runs > 16 and (len(redo) > F // 8 or runs > 64):
        in_place = False
    for f in redo:  # the compact layout of the frame has to fit the frame's own slots
        if sizes[f] + (SLOT_ALIGN - 1) * num_parts + SLOT_ALIGN > t.slots_per_frame:
            in_place = False
    pr.redo = "in-place" if in_place else "whole-batch"
    pr.arena = moved if in_place else 0  # (the whole batch again on the two-pass path: nothing of the first attempt is counted)
    pr.redo_stats = (F, len(redo) if in_place else F)
    pr.one_pass_stats = (1, 1)
    return pr


def resubmitted(F):
    """the same batch again: the rebuilt table holds every count"""
    pr = Prediction()
    pr.redo, pr.arena, pr.redo_stats, pr.one_pass_stats = None, 0, (F, 0), (1, 0)
    return pr


# ---------------------------------------------------------------------------------------------------------------
# the clouds
# ---------------------------------------------------------------------------------------------------------------
def _rows(x, y, z, w=0.5):
    pts = np.empty((len(z), 4), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3] = x, y, z, w
    return pts


def place(rng, p, spec, n):
    """n points of the part `spec`, away from every bin limit, the split height and the RNR rule's thresholds"""
    h = float(p.sensor_height)
    if spec[0] == "rnr":  # low intensity, 1.0-1.5 m below the ground, 17-30 degrees below the horizon
        r, t = rng.uniform(4.0, 8.0, n), rng.uniform(0.0, 2 * math.pi, n)
        return _rows(r * np.cos(t), r * np.sin(t), -h - rng.uniform(1.3, 1.8, n), 0.05)
    if spec[0] == "far":
        r, t = rng.uniform(p.max_range + 5.0, p.max_range + 30.0, n), rng.uniform(0.0, 2 * math.pi, n)
        return _rows(r * np.cos(t), r * np.sin(t), rng.uniform(-2.0, 3.0, n))
    x, y = lo._polar(rng, lo.bin_limits(p, *spec[1:]), n)
    if spec[0] == "hi":
        z = -h + rng.uniform(0.9, 2.0, n)
    elif spec[0] == "lo":
        z = -h + rng.uniform(-0.03, 0.03, n)
    else:  # an unsplit bin: a floor and what stands on it
        z = -h + np.where(rng.uniform(0, 1, n) < 0.7, rng.uniform(-0.03, 0.03, n), rng.uniform(0.3, 1.5, n))
    return _rows(x, y, z)


class Frame:
    """counts: {part spec: points}.  layout "shuffle": rows shuffled; "alternate": the rows of the two parts `pair` alternate, pair
    after pair spread through the cloud; "one-tile": they alternate in one block that starts at a multiple of 1024 rows.
    minus_inf: a part one of whose points gets z = -inf (its bin then needs k_fit_fixup).  edge, delta, want: which limit the frame
    stands at, on which side, and the outcome it is there for."""

    def __init__(self, counts, edge="", delta=0, want="fits", layout="shuffle", pair=None, minus_inf=None):
        self.counts = {k: int(v) for k, v in counts.items() if v > 0}
        self.edge, self.delta, self.want, self.layout, self.pair, self.minus_inf = edge, delta, want, layout, pair, minus_inf

    def n(self):
        return sum(self.counts.values())

    def planned(self, p):
        c = np.zeros(num_parts(p), np.int64)
        for spec, k in self.counts.items():
            c[part_index(p, spec)] += k
        return c

    def key(self):
        return (tuple(sorted(self.counts.items())), self.layout, self.pair, self.minus_inf)

    def cloud(self, p, seed):
        rng = np.random.default_rng(seed)
        blocks = {spec: place(rng, p, spec, k) for spec, k in sorted(self.counts.items())}
        if self.minus_inf is not None:
            blocks[self.minus_inf][0, 2] = -np.inf
        if self.layout == "shuffle":
            pts = np.concatenate(list(blocks.values()), axis=0)
            return np.ascontiguousarray(pts[rng.permutation(len(pts))])
        a, b = (blocks.pop(s) for s in self.pair)
        m = min(len(a), len(b))
        ab = np.empty((2 * m, 4), np.float32)
        ab[0::2], ab[1::2] = a[:m], b[:m]
        rest = np.concatenate(list(blocks.values()) + [a[m:], b[m:]], axis=0)
        rest = rest[rng.permutation(len(rest))]
        if self.layout == "one-tile":
            at = 1024 if len(rest) >= 1024 else 0
            return np.ascontiguousarray(np.concatenate([rest[:at], ab, rest[at:]], axis=0))
        assert self.layout == "alternate"
        out = []
        for i in range(m):
            out += [ab[2 * i: 2 * i + 2], rest[i * len(rest) // m: (i + 1) * len(rest) // m]]
        return np.ascontiguousarray(np.concatenate(out, axis=0))


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
LO0, HI0 = ("lo", 0, 0, 3), ("hi", 0, 0, 3)     # the two parts of one bin of the split zone
Z1, Z2, Z3 = ("bin", 1, 1, 5), ("bin", 2, 1, 7), ("bin", 3, 2, 9)
P0 = ("lo", 0, 0, 0)                            # part 0
LAST = ("bin", 3, 3, 31)                        # the last real part
RNR, FAR = ("rnr",), ("far",)
NEW = ("bin", 2, 2, 20)                         # a part the handle has never seen

BASE = {LO0: 100, HI0: 60, Z1: 80, Z2: 70, Z3: 50, P0: 40, LAST: 30, RNR: 45, FAR: 55}
KINDS = (("low", (LO0,)), ("high", (HI0,)), ("low+high", (LO0, HI0)), ("zone1", (Z1,)), ("zone2", (Z2,)), ("zone3", (Z3,)),
         ("part0", (P0,)), ("last", (LAST,)), ("rnr", (RNR,)), ("far", (FAR,)), ("rnr+far", (RNR, FAR)), ("zone2+far", (Z2, FAR)),
         ("never-seen", (NEW,)))


def scattered_new_parts(p, taken, k):
    """k parts no frame of the sizing batch touches, spread over the whole part range: both sides of split bins, every zone, RNR"""
    specs = []
    for zone in range(4):
        for ring in range(p.num_rings_each_zone[zone]):
            for sector in range(p.num_sectors_each_zone[zone]):
                specs += [("lo", zone, ring, sector), ("hi", zone, ring, sector)] if zone < SPLIT_ZONES else [("bin", zone, ring, sector)]
    bins_taken = {s[1:] for s in taken if len(s) > 1}
    specs = [s for s in specs if s[1:] not in bins_taken]
    pick = [specs[(i * len(specs)) // (k - 1)] for i in range(k - 1)]
    assert len(set(pick)) == k - 1
    return pick + [RNR]


class Built:
    pass


class Case:
    """name; frames per batch; one_pass_scale; debug_flags; the frame every sizing frame is; plan(case, p, table) -> {position: Frame}"""

    def __init__(self, name, frames, base, plan, scale=4.0, debug=0, whole_batch=False, seed=0):
        self.name, self.frames, self.base, self.plan, self.scale, self.debug, self.whole_batch, self.seed = name, frames, Frame(base), plan, scale, debug, whole_batch, seed
        self._built = None

    def __repr__(self):
        return self.name

    def table(self, p, observed, largest):
        return capacity_table(observed, passed_max_n(largest), self.frames, self.scale, split_end(p), num_bins(p), self.debug)

    def built(self, p):
        if self._built is not None:
            return self._built
        b = Built()
        b.observed = self.base.planned(p)
        b.sizing_table = self.table(p, b.observed, self.base.n())
        # the sizing batch itself fits, so nothing is stale when the test batch arrives
        assert outcome(b.observed, b.sizing_table).kind == "fits"
        t = b.sizing_table
        for _ in range(8):  # the counts follow from the table, the table from the largest frame
            plan = self.plan(self, p, t)
            largest = max([self.base.n()] + [f.n() for f in plan.values()])
            rebuild, again = next_table(b.sizing_table, False, largest, self.frames, self.scale)
            assert not again
            t2 = self.table(p, b.observed, largest) if rebuild else b.sizing_table
            if t2.key() == t.key():
                break
            t = t2
        else:
            raise AssertionError("%s: counts and table do not settle" % self.name)
        b.test_table, b.plan = t, plan
        b.specs = [plan.get(i, self.base) for i in range(self.frames)]
        b.counts = [f.planned(p) for f in b.specs]
        b.outcomes = [outcome(c, t) for c in b.counts]
        b.prediction = predict(b.outcomes, [f.n() for f in b.specs], t, num_parts(p), self.whole_batch)
        # the same batch again: every part's true count is among the observed maxima now (k_czm_scan keeps them whether the part was
        # moved or clamped, the redo on the two-pass path too); the table is rebuilt where a part in use grew or a frame was redone
        b.observed_after = np.maximum(b.observed, np.max(b.counts, axis=0))
        stale = b.prediction.redo is not None or any(b.observed_after[q] > b.observed[q] and t.cap[q] > 0 for q in range(len(t.cap)))
        rebuild, again = next_table(t, stale, largest, self.frames, self.scale)
        assert not again
        b.again_table = self.table(p, b.observed_after, largest) if rebuild else t
        b.again_outcomes = [outcome(c, b.again_table) for c in b.counts]
        b.again_prediction = predict(b.again_outcomes, [f.n() for f in b.specs], b.again_table, num_parts(p), self.whole_batch)
        base_cloud = self.base.cloud(p, [self.seed, 999])
        clouds = {}
        b.sizing = [base_cloud] * self.frames
        b.test = []
        for i, f in enumerate(b.specs):  # (identical frames are one array: one oracle run serves them)
            if f is self.base:
                b.test.append(base_cloud)
            else:
                if f.key() not in clouds:
                    clouds[f.key()] = f.cloud(p, [self.seed, i])
                b.test.append(clouds[f.key()])
        self._built = b
        return b


def vary(base, changes):
    c = dict(base.counts)
    c.update(changes)
    return c


def plan_segment_edge(case, p, t):
    """every kind of part at capacity - 1, capacity and capacity + 1; position 0 and the last position move a part, and frames that move
    parts stand next to each other"""
    cap = lambda s: t.cap[part_index(p, s)]
    by_delta = {-1: [], 0: [], 1: []}
    for kind, parts in KINDS:
        for d in (-1, 0, 1):
            by_delta[d].append(Frame(vary(case.base, {s: cap(s) + d for s in parts}), "segment:" + kind, d, "moved" if d > 0 else "fits"))
    seq = [by_delta[1][0]] + by_delta[-1] + [case.base] + by_delta[0] + [case.base] + by_delta[1][1:]
    assert len(seq) == case.frames
    return {i: f for i, f in enumerate(seq) if f is not case.base}


PC_BASE = {Z1: 80, Z3: 50, FAR: 20}


def plan_part_count(counts):
    def plan(case, p, t):
        new = scattered_new_parts(p, case.base.counts, 65)
        out = {}
        for i, k in enumerate(counts):
            out[3 + 5 * i] = Frame(vary(case.base, {s: 33 for s in new[65 - k:]}), "parts", k - MAX_RELOC,
                                   "moved" if k <= MAX_RELOC else "host: too-many-parts")
        return out
    return plan


BIG_BASE = {Z1: 1000, Z2: 1000, Z3: 1000, LO0: 1000, HI0: 1000, FAR: 1000}
NEW5 = (("bin", 1, 3, 2), ("hi", 0, 1, 9), ("bin", 2, 3, 40), ("lo", 0, 1, 12), ("bin", 3, 0, 17))


def plan_spill(deltas, spread):
    def plan(case, p, t):
        out = {}
        for i, d in enumerate(deltas):
            total = t.arena_spill + d
            want = "moved" if d <= 0 else "host: spill-full"
            if not spread:
                ch = {NEW: t.cap[part_index(p, NEW)] + total}
            else:  # five parts never seen take 200 records each, a part seen before the rest
                ch = {s: t.cap[part_index(p, s)] + 200 for s in NEW5}
                ch[Z1] = t.cap[part_index(p, Z1)] + total - 1000
            out[2 + 9 * i] = Frame(vary(case.base, ch), "spill:" + ("spread" if spread else "single"), d, want)
        return out
    return plan


AR_BASE = {Z1: 1000, Z2: 1000, Z3: 1000, FAR: 200}


def plan_arena_room(deltas):
    def plan(case, p, t):
        caps = [t.cap[part_index(p, s)] for s in (Z1, Z2, Z3)]
        out = {}
        for i, d in enumerate(deltas):
            target = t.arena_slots + d
            found = None
            for e3 in (40, 200):
                for e2 in range(33, 700, 32):
                    for e1 in range(1, 900):
                        if align(e1 + e2 + e3) + sum(align(c + e) for c, e in zip(caps, (e1, e2, e3))) == target:
                            found = (e1, e2, e3)
                            break
                    if found:
                        break
                if found:
                    break
            assert found, "no counts land a run of %d" % target
            ch = {s: c + e for s, c, e in zip((Z1, Z2, Z3), caps, found)}
            out[4 + 7 * i] = Frame(vary(case.base, ch), "arena", d, "moved" if d <= 0 else "host: arena-full")
        return out
    return plan


SA_BASE = {Z1: 16, Z2: 16, Z3: 16, LO0: 16, HI0: 16, FAR: 16}


def plan_small_arena(which):
    def plan(case, p, t):
        assert t.arena_slots < 2048 and t.arena_spill == t.arena_slots
        cap = t.cap[part_index(p, Z1)]
        if which == "moved":  # one record; one record in a part never seen; the most records whose part still fits behind them
            most = max(s for s in range(1, t.arena_slots) if align(s) + align(cap + s) <= t.arena_slots)
            return {1: Frame(vary(case.base, {Z1: cap + 1}), "small:one-record", 0, "moved"),
                    6: Frame(vary(case.base, {NEW: 33}), "small:one-record-new", 0, "moved"),
                    11: Frame(vary(case.base, {HI0: t.cap[part_index(p, HI0)] + most}), "small:room", 0, "moved")}
        if which == "room+1":
            most = max(s for s in range(1, t.arena_slots) if align(s) + align(cap + s) <= t.arena_slots)
            more = min(s for s in range(most, t.arena_slots) if align(s) + align(cap + s) > t.arena_slots)
            return {11: Frame(vary(case.base, {HI0: t.cap[part_index(p, HI0)] + more}), "small:room", 1, "host: arena-full")}
        if which == "full":  # records fill the whole arena: no room for the part itself
            return {5: Frame(vary(case.base, {Z1: cap + t.arena_slots}), "small:records", 0, "host: arena-full")}
        return {5: Frame(vary(case.base, {Z1: cap + t.arena_slots + 1}), "small:records", 1, "host: spill-full")}
    return plan


# Parts 63 and 64: neighbours in part order that two different waves of k_czm_scan find overgrown, in either order.  Their membership
# bits (441 bytes each, 64 bytes of pad between neighbours) collide unless the moved parts are placed in part order.
W63, W64 = ("hi", 0, 1, 15), ("bin", 1, 0, 0)
RK_BASE = {LO0: 3000, HI0: 3000, W63: 3000, W64: 3000, P0: 40, Z3: 1500, FAR: 100}  # (two ground patches in the first ring: a lone one sets a stream's sensor height to 0)


def plan_ranks(case, p, t):
    assert (part_index(p, W63), part_index(p, W64)) == (63, 64)
    ch = {s: t.cap[part_index(p, s)] + 200 for s in (LO0, HI0)}
    seam = {s: t.cap[part_index(p, s)] + 200 for s in (W63, W64)}
    return {3: Frame(vary(case.base, ch), "ranks:alternate", 0, "moved", "alternate", (LO0, HI0)),
            7: Frame(vary(case.base, seam), "ranks:wave-seam", 0, "moved"),
            12: Frame(vary(case.base, ch), "ranks:one-tile", 0, "moved", "one-tile", (LO0, HI0))}


def plan_positions(case, p, t):
    cap = lambda s: t.cap[part_index(p, s)]
    return {0: Frame(vary(case.base, {Z1: cap(Z1) + 3}), "position:first", 0, "moved"),
            8: Frame(vary(case.base, {HI0: cap(HI0) + 2, FAR: cap(FAR) + 5}), "position:adjacent", 0, "moved"),
            9: Frame(vary(case.base, {LO0: cap(LO0) + 7, NEW: 40}), "position:adjacent", 0, "moved"),
            case.frames - 1: Frame(vary(case.base, {LAST: cap(LAST) + 9, RNR: cap(RNR) + 1}), "position:last", 0, "moved")}


def plan_two_ranges(case, p, t):
    """130 frames run as two frame ranges on two streams: frames that move parts in each range, at the seam and at both ends"""
    f = plan_positions(case, p, t)
    return {0: f[0], 40: f[8], 64: f[9], 65: f[8], 100: f[0], case.frames - 1: f[case.frames - 1]}


NA_BASE = {Z1: 1000, Z2: 1000, Z3: 800, FAR: 100}


def plan_no_arena(want):
    def plan(case, p, t):  # a part never seen takes one point more than the segment of a few-frames table holds
        return {5: Frame(vary(case.base, {NEW: 2049}), "no-arena", 0, want), 6: Frame(vary(case.base, {NEW: 2049, Z3: 700}), "no-arena", 0, want)}
    return plan


def plan_fixup(case, p, t):
    # (beyond the first zone: there the seed selection skips heights far below the sensor, -inf among them, and no fix-up is needed)
    return {7: Frame(vary(case.base, {LO0: t.cap[part_index(p, LO0)] + 1, Z1: t.cap[part_index(p, Z1)] + 1}), "fixup", 0, "moved", minus_inf=Z1)}


IP_BASE = {Z3: 12000, Z1: 500, FAR: 100}


def plan_in_place(case, p, t):
    new = scattered_new_parts(p, case.base.counts, 65)
    return {4: Frame(vary(case.base, {s: 33 for s in new}), "parts", 1, "host: too-many-parts"),
            10: Frame(vary(case.base, {Z1: t.cap[part_index(p, Z1)] + 1}), "segment:zone1", 1, "moved")}


def make_cases():
    return [
        Case("segment-edge", 41, BASE, plan_segment_edge, seed=1),
        Case("part-count-63-64", 17, PC_BASE, plan_part_count((63, 64)), seed=2),
        Case("part-count-65", 17, PC_BASE, plan_part_count((65,)), seed=3),
        Case("spill-single", 20, BIG_BASE, plan_spill((-1, 0), False), seed=4),
        Case("spill-single+1", 17, BIG_BASE, plan_spill((1,), False), seed=5),
        Case("spill-spread", 20, BIG_BASE, plan_spill((-1, 0), True), seed=6),
        Case("spill-spread+1", 17, BIG_BASE, plan_spill((1,), True), seed=7),
        Case("arena-room", 17, AR_BASE, plan_arena_room((-32, 0)), seed=8),
        Case("arena-room+32", 17, AR_BASE, plan_arena_room((32,)), seed=9),
        Case("small-arena-moved", 17, SA_BASE, plan_small_arena("moved"), scale=0.25, seed=10),
        Case("small-arena-room+1", 17, SA_BASE, plan_small_arena("room+1"), scale=0.25, seed=11),
        Case("small-arena-records", 17, SA_BASE, plan_small_arena("full"), scale=0.25, seed=12),
        Case("small-arena-records+1", 8, SA_BASE, plan_small_arena("full+1"), scale=0.25, seed=13),
        Case("ranks", 17, RK_BASE, plan_ranks, seed=14),
        Case("positions", 17, BASE, plan_positions, seed=15),
        Case("arena-17", 17, NA_BASE, plan_no_arena("moved"), seed=16),
        Case("few-16", 16, NA_BASE, plan_no_arena("host: no-arena"), seed=16),
        Case("debug-2048", 17, NA_BASE, plan_no_arena("host: no-arena"), debug=NO_ARENA_FLAG, seed=16),
        Case("fixup", 17, BASE, plan_fixup, seed=17),
        Case("redo-in-place", 17, IP_BASE, plan_in_place, seed=18),
        Case("two-ranges", 130, BASE, plan_two_ranges, seed=19),
    ]


CASES = make_cases()
# the cases whose frames are also checked list by list, output by output, as streams and in a batch of two frame ranges
DEEP = ("segment-edge", "ranks", "part-count-65")


def rows_of_table(p):
    """the account of the cases: one row per planned frame (profiles/one_pass_arena_cases.txt)"""
    rows = []
    for case in CASES:
        b = case.built(p)
        t = b.test_table
        for i in sorted(b.plan):
            f, o, c = b.specs[i], b.outcomes[i], b.counts[i]
            base = case.base.planned(p)
            at = [q for q in range(len(c)) if c[q] != base[q]]
            edge = " ".join("%s:%d/%d" % (part_name(p, q), c[q], t.cap[q]) for q in at[:4]) + (" +%d more" % (len(at) - 4) if len(at) > 4 else "")
            rows.append("%-22s %2d %-22s %+3d  n=%-5d %-44s nov %2d/%d spilled %4d/%d run %4d/%d  %-20s | %s"
                        % (case.name, i, f.edge, f.delta, f.n(), edge, o.nov, MAX_RELOC, o.spilled, t.arena_spill, o.run, t.arena_slots, o, b.prediction))
    return rows
