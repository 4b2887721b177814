"""The cooperative wide walk's list discipline (csrc/hip/rt_coop.h: coop_push_rays, coop_trace, coop_make_room), restated exactly at wave level:
the node ring in LDS with its head, the arena block the ring spills to, the leaf stack, the counters the kernel keeps (CoopCount) and the
overflow rule (coop_overflow).  What it does not restate is what the lists carry no trace of: the leaf trips' primitive tests (only how many
records each popped item brings decides a trip's pops) and the shadow rays' any-hit drops (the probe traces extension rays only; the pool's
batches are modelled without drops, which only ever take items away).  Each trip is one vectorised step over the items it pops, in the
kernel's order: lanes in order, a node's child slots k = 0..3 one after the other, interior children before the hit leaves.

The slab test is the kernel's float32 expression: inv = the IEEE quotient 1 / d, (box - o) * inv per axis, np.fmin / np.fmax for
__builtin_fminf / fmaxf (the non-NaN operand wins, where np.minimum would propagate a NaN), t0 clamped at 0, t1 at inf, hit = !(t0 > t1)."""
import numpy as np

NCAP = 320        # RT_COOP_NCAP: node-ring entries in LDS
LCAP = 320        # RT_COOP_LCAP: leaf-stack entries
GCAP = 4096       # RT_COOP_GCAP: node items a wave may spill (the arena block's size)
LIFO_AT = 512     # RT_COOP_LIFO_AT
NARROW_AT = 3072  # RT_COOP_NARROW_AT
MIN_LDS_CAP = 64  # RT_COOP_MIN_LDS_CAP
SLOT_SHIFT = 25   # 32 - RT_COOP_SLOT_BITS
KIND = 1 << 24    # RT_COOP_KIND: the slot's shadow ray
HEAD = ~(KIND - 1) & 0xFFFFFFFF
NODE_MASK = KIND - 1

COUNTERS = ("node_trips", "leaf_trips", "spills", "refills", "lifo_trips", "narrow_trips", "overflows", "peak")  # rsrt_get_walk_counters


class Tree:
    """A wide tree as rsrt_wide_tree_build lays it out ((n, 8, 4) float32): per node the four child boxes, the interior-slot mask, the first
    interior child, and each slot's record count (the popcount of its record mask; 0: not a leaf)."""

    def __init__(self, wn):
        w = wn.view(np.uint32)
        self.n = len(wn)
        self.lo = np.ascontiguousarray(wn[:, 0::2, :3])  # (n, 4, 3)
        self.hi = np.ascontiguousarray(wn[:, 1::2, :3])
        wa = w[:, 0, 3].astype(np.int64)
        self.imask = wa >> 26
        self.child0 = wa & 0x3FFFFFF
        masks = w[:, 4:8, 3].astype(np.int64)
        self.nrec = np.zeros_like(masks)
        for b in range(32):
            self.nrec += (masks >> b) & 1
        self.depth = self._depth()
        self.imask_l, self.child0_l, self.nrec_l = self.imask.tolist(), self.child0.tolist(), self.nrec.tolist()  # (one-item trips)

    def _depth(self):
        lv = np.zeros(self.n, np.int64)
        lv[0] = 1
        for i in range(self.n):  # (children come after their parent)
            for k in range(int(self.imask[i]).bit_length()):
                lv[self.child0[i] + k] = lv[i] + 1
        return int(lv.max())


def ray_ok(o, d):
    """coop_ray_ok: every component of d has a biased exponent in 2..252 (the short reciprocal is the IEEE quotient there) and o is finite."""
    e = (np.ascontiguousarray(d, np.float32).view(np.uint32) >> 23) & 0xFF
    short_ok = ((e.astype(np.int64) - 2) & 0xFFFFFFFF) < 251
    o = np.asarray(o, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = ((o[:, 0] + o[:, 1]) + o[:, 2]) * np.float32(0) == 0
    return short_ok.all(axis=1) & fin


def hit_masks(tree, o, d):
    """The 4-bit child hit mask of every (ray, node): (n_rays, n_nodes) uint8, by the kernel's float32 slab test."""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv = (np.float32(1) / d).astype(np.float32)
        out = np.zeros((len(o), tree.n), np.uint8)
        step = max(1, (1 << 20) // max(1, 4 * tree.n))
        for r0 in range(0, len(o), step):
            oo, ii = o[r0:r0 + step, None, None, :], inv[r0:r0 + step, None, None, :]
            a = (tree.lo[None] - oo) * ii  # (rays, nodes, 4, 3), float32 throughout
            b = (tree.hi[None] - oo) * ii
            mn, mx = np.fmin(a, b), np.fmax(a, b)
            t0 = np.fmax(np.fmax(np.fmax(mn[..., 0], mn[..., 1]), mn[..., 2]), np.float32(0))
            t1 = np.fmin(np.fmin(np.fmin(mx[..., 0], mx[..., 1]), mx[..., 2]), np.float32(np.inf))
            hit = ~(t0 > t1)
            out[r0:r0 + step] = (hit * np.uint8([1, 2, 4, 8])).sum(axis=-1)
    return out


class Wave:
    """One wave's lists and counters, run over one batch.  hm: hit masks of the batch's rays (row = slot, or n_slots + slot for the
    slot's shadow ray)."""

    def __init__(self, tree, hm, n_slots, lds_cap=NCAP, lifo_at=LIFO_AT, narrow_at=NARROW_AT, gcap=GCAP):
        self.t, self.hm, self.n_slots = tree, hm, n_slots
        self.lds_cap, self.lifo_at, self.narrow_at, self.gcap = lds_cap, lifo_at, narrow_at, gcap
        self.ns = np.zeros(NCAP, np.int64)
        self.ns_h = self.ns_n = 0
        self.gs = np.zeros(GCAP, np.int64)
        self.gs_n = 0
        self.ls = np.zeros(LCAP, np.int64)  # the record count of each leaf item
        self.ls_n = 0
        self.overflow = False
        self.c = dict.fromkeys(COUNTERS, 0)
        self.most = {"ring": 0, "arena": 0, "leaf": 0}

    def ring(self, i):  # CoopStacks::ring (i < 2 * NCAP - head)
        k = self.ns_h + np.asarray(i, np.int64)
        assert (k < 2 * NCAP).all()
        return np.where(k >= NCAP, k - NCAP, k)

    def _push(self, items):  # ring_new, lane after lane
        assert self.ns_n + len(items) <= NCAP  # what the kernel's guard makes sure of
        self.ns[self.ring(self.ns_n + np.arange(len(items)))] = items
        self.ns_n += len(items)
        self.most["ring"] = max(self.most["ring"], self.ns_n)

    def _make_room(self, n_new):
        while self.ns_n + n_new > self.lds_cap and self.ns_n >= 64 and self.gs_n + 64 <= self.gcap:
            self.ns_n -= 64
            self.gs[self.gs_n:self.gs_n + 64] = self.ns[self.ring(self.ns_n + np.arange(64))]
            self.gs_n += 64
            self.c["spills"] += 1
            self.most["arena"] = max(self.most["arena"], self.gs_n)

    def _overflow(self):
        self.overflow = True
        self.ns_n = self.gs_n = self.ls_n = 0
        self.c["overflows"] += 1

    def push_rays(self, slots, push_e, push_s):
        """coop_push_rays for one chunk of up to 64 lanes: lane i names slots[i]; push_e / push_s: which of its rays go on the ring."""
        if self.ns_n + 128 > self.lds_cap:
            self._make_room(128)
        slots = np.asarray(slots, np.int64)
        e, s = slots[np.asarray(push_e, bool)], slots[np.asarray(push_s, bool)]
        if self.overflow:
            return
        if self.ns_n + len(e) + len(s) > NCAP:
            self._overflow()
            return
        self._push(e << SLOT_SHIFT)
        self._push((s << SLOT_SHIFT) | KIND)

    def trace(self):
        """coop_trace: trips until the lists are dry."""
        t = self.t
        lanes = np.arange(64)
        while True:
            if self.ls_n >= 64 or (self.ns_n == 0 and self.gs_n == 0 and self.ls_n != 0):
                # leaf trip: lane i pops the i-th item from the top; the items whose records end within the first 128 are taken
                self.c["leaf_trips"] += 1
                n_take = min(self.ls_n, 64)
                cnt = self.ls[self.ls_n - 1 - lanes[:n_take]]
                end = np.cumsum(cnt)
                self.ls_n -= int((end <= 128).sum())
                continue
            if self.ns_n < 64 and self.gs_n != 0:  # refill: the arena's newest block comes back behind the ring's fill
                self.gs_n -= 64
                self.ns[self.ring(self.ns_n + lanes)] = self.gs[self.gs_n:self.gs_n + 64]
                self.ns_n += 64
                self.c["refills"] += 1
                self.most["ring"] = max(self.most["ring"], self.ns_n)
            if self.ns_n == 0:
                break
            n_out = self.ns_n + self.gs_n
            narrow = n_out > self.narrow_at
            newest = narrow or n_out > self.lifo_at
            n_take = 1 if narrow else min(self.ns_n, 64)
            self.c["node_trips"] += 1
            self.c["lifo_trips"] += newest
            self.c["narrow_trips"] += narrow
            self.c["peak"] = max(self.c["peak"], n_out)
            if newest:
                items = self.ns[self.ring(self.ns_n - 1 - lanes[:n_take])]
            else:
                items = self.ns[self.ring(lanes[:n_take])]
                self.ns_h = int(self.ring(n_take))
            self.ns_n -= n_take
            if n_take == 1:  # (the same trip for one item, in plain Python: one-item trips come by the ten thousand)
                it = int(items[0])
                nd, row = it & NODE_MASK, (it >> SLOT_SHIFT) + (self.n_slots if it & KIND else 0)
                h = int(self.hm[row, nd])
                im, c0, nr = h & self.t.imask_l[nd], self.t.child0_l[nd], self.t.nrec_l[nd]
                new = [(it & HEAD) | (c0 + k) for k in range(4) if (im >> k) & 1]
                leaves = [nr[k] for k in range(4) if (h >> k) & 1 and nr[k] > 0]
            else:
                new, leaves = self._expand(items)
            if self.ns_n + len(new) > self.lds_cap:
                self._make_room(len(new))
            if self.ns_n + len(new) > NCAP:
                self._overflow()
                continue
            self._push(np.asarray(new, np.int64))
            assert self.ls_n + len(leaves) <= LCAP
            self.ls[self.ls_n:self.ls_n + len(leaves)] = leaves
            self.ls_n += len(leaves)
            self.most["leaf"] = max(self.most["leaf"], self.ls_n)
        return self

    def _expand(self, items):
        """A node trip's pushes for the items it popped, in the kernel's order: the hit interior children slot by slot (k = 0..3, lanes in
        order within a slot), then the hit leaves the same way."""
        t = self.t
        node = items & NODE_MASK
        row = (items >> SLOT_SHIFT) + np.where(items & KIND, self.n_slots, 0)
        hm = self.hm[row, node].astype(np.int64)
        im = hm & t.imask[node]
        head = items & HEAD
        new = np.concatenate([head[(im >> k) & 1 == 1] | (t.child0[node[(im >> k) & 1 == 1]] + k) for k in range(4)])
        leaves = np.concatenate([t.nrec[node, k][((hm >> k) & 1 == 1) & (t.nrec[node, k] > 0)] for k in range(4)])
        return new, leaves


def add(total, c):
    """Counters of another wave into `total` (peak: a maximum, the rest sums) — what the kernels' flush does."""
    for k in COUNTERS:
        total[k] = max(total[k], c[k]) if k == "peak" else total[k] + c[k]
    return total


def probe(tree, o, d, **knobs):
    """rsrt_cast_rays through the cooperative walk (rt_cast_rays_coop_kernel): 64 rays a wave, by index, extension rays only.
    Returns (counters summed over the waves, the most any wave's ring / arena / leaf stack held)."""
    total, most = dict.fromkeys(COUNTERS, 0), {"ring": 0, "arena": 0, "leaf": 0}
    ok = ray_ok(o, d)
    for w0 in range(0, len(o), 64):
        n = min(64, len(o) - w0)
        wv = Wave(tree, hit_masks(tree, o[w0:w0 + n], d[w0:w0 + n]), 64, **knobs)
        wv.push_rays(np.arange(n), ok[w0:w0 + n], np.zeros(n, bool))
        wv.trace()
        add(total, wv.c)
        most = {k: max(most[k], wv.most[k]) for k in most}
    return total, most


def pool_batch(tree, o, d_ext, d_shadow, pool=128, hm=None, **knobs):
    """One TRACE call of the render kernel (rt_wavepool.h, TRAV 6): a pool of up to 128 slots, each with an extension and a shadow ray,
    pushed in chunks of 64 slots.  hm: the hit masks of the 2 * pool rays, if already at hand.  Returns the wave."""
    n = len(o)
    assert n <= pool
    if hm is None:
        hm = np.zeros((2 * pool, tree.n), np.uint8)
        hm[:n] = hit_masks(tree, o, d_ext)
        hm[pool:pool + n] = hit_masks(tree, o, d_shadow)
    wv = Wave(tree, hm, pool, **knobs)
    ok_e, ok_s = ray_ok(o, d_ext), ray_ok(o, d_shadow)
    for i0 in range(0, n, 64):
        sl = np.arange(i0, min(n, i0 + 64))
        wv.push_rays(sl, ok_e[sl], ok_s[sl])
    return wv.trace()


DECK_LEVELS = 74  # the deepest util.deck_scene whose wide tree qualifies: 25 wide levels, build_wide_tree's limit (test_wide_tree.py checks)
FAN_QUADS = 256  # util.fan_scene: 85 wide nodes in 4 levels, every one hit by every ray of batch_rays("along", ...)
PEAK_BOUND = 2048  # most node items a wave may hold outstanding by rt_coop.h's header (the sweep's worst is well below; RT_COOP_GCAP / 2)

# the knob sets the tests sweep: RSRT_COOP_LDS_CAP x RSRT_COOP_LIFO_AT x RSRT_COOP_NARROW_AT (the defaults among them)
KNOBS = [dict(lds_cap=c, lifo_at=f, narrow_at=n) for c in (64, 128, 320) for f in (0, 64, 512, 3072) for n in (0, 40, 3072)]


def batch_rays(kind, wn, n, seed):
    """n rays for a batch: "along" — from z = 3 down the -z axis with a little spread (util.deck_scene, util.fan_scene: every box is met);
    otherwise aimed from a box around the tree's root box at random points inside it (suzanne, the grid: most rays meet the mesh)."""
    rng = np.random.default_rng(seed)
    if kind == "along":
        o = (rng.uniform(-0.5, 0.5, (n, 3)) + [0, 0, 3]).astype(np.float32)
        d = (rng.normal(size=(n, 3)) * 0.05 + [0, 0, -1]).astype(np.float32)
    else:
        lo, hi = wn[0, 0::2, :3].min(axis=0), wn[0, 1::2, :3].max(axis=0)
        c, r = (lo + hi) / 2, (hi - lo) / 2
        o = (c + r * rng.uniform(-1.5, 1.5, (n, 3))).astype(np.float32)
        d = (c + r * rng.uniform(-0.6, 0.6, (n, 3)) - o).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)
