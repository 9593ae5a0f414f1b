"""The multi-rank context exchange (csrc/sync.hip, csrc/exchange.hip) restated in plain numpy, ALL ranks in one process (test
infrastructure; no torch, no torch.distributed, nothing of tests/sync_model.py).

Written from the comments and the arithmetic of the two files: every fp32 operation of a kernel is one numpy float32 operation here,
in the kernel's order (the library is built with -ffp-contract=off, so there is nothing fused to restate), and the group's sums are
the local group's: from 0.0f, in rank order.  What the model holds, per rank, is what a rank holds on the device -- the four
context-side tables, and per table the base (the consensus c), the delta in flight (own) and, for the mean rule, the counts --
so a test can compare the tables word for word after every call and the model's own tests can look at the parts a device hides.

`fault=` makes the model wrong in ONE named way (FAULTS): tests/test_exchange_ref.py uses it to prove that the designed tables below
can see such a fault at all; the GPU tests never pass it."""
import numpy as np

F = np.float32
M32 = np.uint64(0xFFFFFFFF)
NAMES = ("context", "cbias", "gsq_context", "gsq_cbias")       # get_state / set_state names, in the order ge_sync_create adds its entries
FAULTS = ("no_feedback", "truncate", "ties_away", "swap_halves", "base_not_landed", "mean_by_world", "lazy_wrong_calls", "skip_tail")
FAULTS_BF16_ROWS = ("rne_on_land", "hub_from_bf16")


# ---- number formats ------------------------------------------------------------------------------------------------------
def narrow(x, mode="rne"):
    """f32_to_bf16_rne: (u + 0x7fff + ((u >> 16) & 1)) >> 16, a NaN stays a NaN through (u >> 16) | 0x40.  (mode: the faults)
    uint32 arithmetic as on the device: the sum wraps only for words that are NaNs, which take the other branch."""
    u = np.ascontiguousarray(x, F).view(np.uint32)
    hi = u >> np.uint32(16)
    if mode == "rne":
        r = (u + (np.uint32(0x7FFF) + (hi & np.uint32(1)))) >> np.uint32(16)
    elif mode == "truncate":
        r = hi
    else:                                                       # "ties_away": round half away from zero
        r = (u + np.uint32(0x8000)) >> np.uint32(16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    if nan.any():
        r = np.where(nan, hi | np.uint32(0x40), r)
    return r.astype(np.uint16)


def narrow_plain(x):
    """ge_glove_set_state on a bf16 table (k_f32_to_bf16): the same rounding without the NaN branch."""
    u = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    return (((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16)


def widen(h):
    return (np.asarray(h).astype(np.uint32) << np.uint32(16)).view(F)


def mix32(x):
    """mix32 / hub_mix32 of the two files (the same function) on uint32 values held in uint64."""
    x = np.asarray(x).astype(np.uint64) & M32
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x85EBCA77)) & M32
    x = x ^ (x >> np.uint64(13)); x = (x * np.uint64(0xC2B2AE3D)) & M32
    return x ^ (x >> np.uint64(16))


def narrow_hashed(x, index, seed):
    """A landed value stored as bf16: bits + (mix32(index * 0x9E3779B1 + seed) >> 16), truncated; an exponent of all ones passes through."""
    bits = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    rnd = mix32((np.asarray(index).astype(np.uint64) * np.uint64(0x9E3779B1) + np.uint64(seed)) & M32) >> np.uint64(16)
    special = (bits & np.uint64(0x7F800000)) == np.uint64(0x7F800000)
    return (np.where(special, bits >> np.uint64(16), ((bits + rnd) & M32) >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16)


def next_seed(seed):
    return (seed * 1664525 + 1013904223) & 0xFFFFFFFF


def rank_seed(seed, rank):
    return seed ^ ((rank * 0x9E3779B1) & 0xFFFFFFFF)


def sqrt_f32(x):
    """A correctly rounded fp32 square root: the fp64 one rounded once more (53 >= 2 * 24 + 2 bits: no double rounding)."""
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.asarray(x, F).astype(np.float64)).astype(F)


# ---- the group's sums (LocalCollective) -----------------------------------------------------------------------------------
def group_sum_f32(parts):
    a = np.zeros(np.shape(parts[0]), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for x in parts:                                         # a = 0.0f; for r in rank order: a += x_r
            a = a + np.asarray(x, F)
    return a


def group_sum_bf16(parts):
    return narrow(group_sum_f32([widen(h) for h in parts]))     # widened, summed in fp32 in rank order, rounded to nearest even


def merge_scale(g0, e_sum, inv_world):
    """sqrt((G0 + E * inv_world) / (G0 + E)) with E = fmaxf(e_sum, 0), operation for operation; inv_world <= 0: 1."""
    if not inv_world > 0:
        return np.ones(np.shape(g0), F)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e = np.fmax(np.asarray(e_sum, F), F(0))
        return sqrt_f32((g0 + e * F(inv_world)) / (g0 + e))


# ---- one turn of one entry on one rank ----------------------------------------------------------------------------------
def turn_f32_table(table, base, wire, own, cnt, land, take, w16, mean, world=0, fault=None):
    """k_sync_turn / k_sync_turn_flat4 on dense arrays (the row stride is the kernel's business):
         land:  c += m (m = wire, or wire / max(cnt, 1) under the mean rule);  resid = (table - c_old) - own;  table = c + resid
         take:  own = narrow(resid) (fp32 wire: resid);  mean rule: cnt = (own != 0)
    Returns (table, base, own, cnt); nothing is changed in place."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = base
        resid = table - c
        if land:
            w, o = (widen(wire), widen(own)) if w16 else (wire, own)
            if mean:
                w = w / (np.full_like(cnt, world) if fault == "mean_by_world" else np.fmax(cnt, F(1)))
            c = c + w
            if fault != "no_feedback":
                resid = resid - o                               # this rank's sent delta is inside w now
            table = c + resid
            if fault != "base_not_landed":
                base = c
        if take:
            if w16:
                own = narrow(resid, fault if fault in ("truncate", "ties_away") else "rne")
                if fault == "swap_halves" and own.size % 2 == 0:
                    own = own.reshape(-1, 2)[:, ::-1].reshape(-1).copy()
                sent = widen(own)
            else:
                own = sent = resid.copy()
            if mean:
                cnt = (sent != 0).astype(F)
    return table, base, own, cnt


def turn_bf16_rows(t16, hub_rows, hub_index, D, base, wire, own, land, take, seed, fault=None):
    """k_exchange_turn_bf16 on a dense bf16 table [V x D] with fp32 master rows hub_rows[hub_index[v]] where hub_index[v] >= 0:
         value = the master row, else the widened table entry;  d = value - base (before landing)
         land:  r = wire - own;  value += r;  base += r;  an ordinary row is stored with narrow_hashed(value, flat index, seed), a hub
                row in its master (its bf16 copy is not touched)
         take:  own = narrow(d);  base += own
    Returns (t16, hub_rows, base, own)."""
    V = hub_index.shape[0]
    is_hub = np.repeat(hub_index >= 0, D)
    hpos = (np.repeat(hub_index.astype(np.int64), D) * D + np.tile(np.arange(D), V))[is_hub]
    t = widen(t16).copy()
    if fault != "hub_from_bf16":
        t[is_hub] = hub_rows[hpos]
    b = base
    with np.errstate(invalid="ignore", over="ignore"):
        d = t - b
        if land:
            r = widen(wire) - widen(own)
            tn = t + r
            b = b + r
            stored = narrow(tn) if fault == "rne_on_land" else narrow_hashed(tn, np.arange(t.size, dtype=np.uint64), seed)
            t16 = np.where(is_hub, t16, stored)
            hub_rows = hub_rows.copy(); hub_rows[hpos] = tn[is_hub]
        if take:
            own = narrow(d)
            b = b + widen(own)
    return t16, hub_rows, b, own


# ---- all ranks -----------------------------------------------------------------------------------------------------------------
class Exchange:
    """ge_sync of `world` ranks.  tables[r] = rank r's four context-side tables (NAMES -> dense fp32 arrays, as get_state shows them)
    at the moment ge_sync_create runs: they become the bases.  rows="bf16": the context rows are a bf16 table with fp32 master rows
    where masters[r][v] (bool [V]: column v is a hub ON rank r); get() / set() then act as ge_glove_get_state / set_state do.
    hubs: the rows of ge_sync_hub_exchange (ascending; what ge_sync_hub_rows returns)."""

    def __init__(self, tables, V, D, wire="bf16", accum_every=4, rows="f32", masters=None, hubs=(), fault=None):
        self.world, self.V, self.D, self.fault = len(tables), int(V), int(D), fault
        self.rows16 = rows == "bf16"
        self.accum_every = int(accum_every) if accum_every else 4
        self.calls, self.seed = 0, 0x5EED
        self.hubs = np.asarray(hubs, np.int64)
        self.inv_world = F(1.0) / F(self.world)
        W = range(self.world)
        self.masters = [np.zeros(V, bool) if masters is None else np.asarray(masters[r], bool) for r in W]
        self.t = [{k: np.array(tables[r][k], F).reshape(-1) for k in NAMES} for r in W]
        if self.rows16:                                          # the stored bf16 table; self.t[r]["context"] holds the master rows' values
            self.t16 = [narrow_plain(self.t[r]["context"]) for r in W]
        w16 = wire == "bf16"
        # ge_sync_create: context rows, cBias (mean: always fp32 on the wire), gradSqContext (lazy), gradSqCBias (lazy, fp32)
        self.ent = [dict(name="context", mean=False, lazy=False, w16=w16 or self.rows16, rows16=self.rows16),
                    dict(name="cbias", mean=True, lazy=False, w16=False, rows16=False),
                    dict(name="gsq_context", mean=False, lazy=True, w16=w16, rows16=False),
                    dict(name="gsq_cbias", mean=False, lazy=True, w16=False, rows16=False)]
        for e in self.ent:
            e["base"] = [self.get(r, e["name"]).copy() for r in W]           # the base is the table NOW
            n = e["base"][0].size
            e["own"] = [np.zeros(n, np.uint16 if e["w16"] else F) for r in W]
            e["cnt"] = [np.zeros(n, F) for r in W]
            e["wire"] = [np.zeros(n, np.uint16 if e["w16"] else F) for r in W]
            e["in_flight"] = False
            e["sent"] = [None] * self.world                      # the residual each rank's last take narrowed (the model's tests read it) ...
            e["sent_base"] = [None] * self.world                 # ... the consensus it was measured against, and the call that took it
            e["taken_at"] = 0
        self.entry = {e["name"]: e for e in self.ent}

    # -- the tables as a host sees them --
    def _mask(self, r):
        return np.repeat(self.masters[r], self.D)

    def get(self, r, name):
        if name == "context" and self.rows16:
            return np.where(self._mask(r), self.t[r]["context"], widen(self.t16[r]))
        return self.t[r][name]

    def set(self, r, name, values):
        v = np.array(values, F).reshape(-1)
        self.t[r][name] = v                                      # (bf16 rows: the master rows take the fp32 value ...
        if name == "context" and self.rows16:
            self.t16[r] = narrow_plain(v)                        #  ... and EVERY row's bf16 entry its rounding)

    def tables(self, r):
        return {k: self.get(r, k).copy() for k in NAMES}

    # -- ge_sync_begin / finish / turn / sync / replicate --
    def _launch(self, e, r, land, take, seed):
        name = e["name"]
        if e["rows16"]:
            hub_index = np.where(self.masters[r], 0, -1).astype(np.int64)       # the model keeps master rows in place: index = the row
            hub_index[self.masters[r]] = np.nonzero(self.masters[r])[0]
            t16, hub, base, own = turn_bf16_rows(self.t16[r], self.t[r][name], hub_index, self.D, e["base"][r], e["wire"][r], e["own"][r],
                                                 land, take, rank_seed(seed, r), self.fault)
            if take:
                e["sent"][r] = None
            self.t16[r], self.t[r][name], e["base"][r], e["own"][r] = t16, hub, base, own
            return
        n = self.t[r][name].size
        stop = n
        if self.fault == "skip_tail" and e["w16"]:               # the last partial group of 1024 elements (a whole one, if none is partial)
            stop = n - (n % 1024 or min(n, 1024))
        s = slice(0, stop)
        if take and e["w16"]:
            with np.errstate(invalid="ignore", over="ignore"):
                resid = self.t[r][name] - e["base"][r]
                if land and self.fault != "no_feedback":
                    resid = resid - widen(e["own"][r])
            e["sent"][r] = resid
        tab, base, own, cnt = turn_f32_table(self.t[r][name][s], e["base"][r][s], e["wire"][r][s], e["own"][r][s], e["cnt"][r][s], land, take,
                                             e["w16"], e["mean"], self.world, self.fault)
        for arr, new in ((self.t[r][name], tab), (e["base"][r], base), (e["own"][r], own), (e["cnt"][r], cnt)):
            arr[s] = new
        if take and e["w16"]:
            e["sent_base"][r] = e["base"][r].copy()

    def _turn(self, land, take, everything=False):
        if self.world == 1:
            return
        due = False
        if take:
            self.calls += 1
            due = everything or self.calls % max(1, self.accum_every) == (1 % max(1, self.accum_every) if self.fault == "lazy_wrong_calls" else 0)
        if take and not land and any(e["in_flight"] for e in self.ent):
            raise RuntimeError("ge_sync: finish the exchange in flight first")
        taken = []
        for e in self.ent:
            do_land, do_take = land and e["in_flight"], take and (due or not e["lazy"])
            if not (do_land or do_take):
                continue
            if e["rows16"]:
                self.seed = next_seed(self.seed)                 # the same sequence on every rank, a new draw per turn
            for r in range(self.world):
                self._launch(e, r, do_land, do_take, self.seed)
            if do_land:
                e["in_flight"] = False
            if do_take:
                taken.append(e)
                e["taken_at"] = self.calls
        for e in taken:                                          # the all-reduce of every entry taken in this call
            total = group_sum_bf16(e["own"]) if e["w16"] else group_sum_f32(e["own"])
            e["wire"] = [total.copy() for r in range(self.world)]
            if e["mean"]:
                cnt = group_sum_f32(e["cnt"])
                e["cnt"] = [cnt.copy() for r in range(self.world)]
            e["in_flight"] = True

    def begin(self, everything=False): self._turn(False, True, everything)
    def finish(self): self._turn(True, False)
    def turn(self): self._turn(True, True)

    def sync(self):
        self._turn(True, True)
        self._turn(True, False)

    def replicate(self, src=0):
        if self.world == 1:
            return
        self._turn(True, True, True)                             # land what is in flight, send everything not sent yet
        self._turn(True, False)
        for e in self.ent:                                       # every rank takes rank src's replica, table and base (bf16 rows: left as landed)
            if e["rows16"]:
                continue
            for r in range(self.world):
                self.t[r][e["name"]] = self.t[src][e["name"]].copy()
                e["base"][r] = self.t[src][e["name"]].copy()

    # -- ge_sync_hub_exchange --
    def hub_exchange(self):
        """k_hub_take, one fp32 sum of buf = [rows H x D | accumulator rows H x D | gradSqCBias H | cBias H | count H], k_hub_land."""
        H, D, W = len(self.hubs), self.D, range(self.world)
        if self.world == 1 or H == 0:
            return
        er, eb, ea, eab = self.ent
        el = (self.hubs[:, None] * D + np.arange(D)[None, :]).reshape(-1)       # the hub rows' elements in the dense tables
        bufs = []
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for r in W:
                if self.rows16:
                    val = widen(self.t16[r])[el] if self.fault == "hub_from_bf16" else self.get(r, "context")[el]
                else:
                    val = self.t[r]["context"][el]
                db = self.t[r]["cbias"][self.hubs] - eb["base"][r][self.hubs]
                bufs.append(np.concatenate([val - er["base"][r][el], self.t[r]["gsq_context"][el] - ea["base"][r][el],
                                            self.t[r]["gsq_cbias"][self.hubs] - eab["base"][r][self.hubs], db, (db != 0).astype(F)]))
            buf = group_sum_f32(bufs)
            self.seed = next_seed(self.seed)
            b_rows, b_acc = buf[:H * D], buf[H * D:2 * H * D]
            b_accb, b_bias, b_cnt = (buf[2 * H * D + k * H:2 * H * D + (k + 1) * H] for k in range(3))
            for r in W:
                c = er["base"][r][el] + merge_scale(ea["base"][r][el], b_acc, self.inv_world) * b_rows
                er["base"][r][el] = c
                if self.rows16:
                    m = np.repeat(self.masters[r][self.hubs], D)                 # the fp32 master where the column is a hub on this rank ...
                    self.t[r]["context"][el[m]] = c[m]
                    hashed = narrow_hashed(c, np.arange(H * D, dtype=np.uint64), rank_seed(self.seed, r))
                    self.t16[r][el[~m]] = hashed[~m]                              # ... else the bf16 entry, index h * D + d of the LIST
                else:
                    self.t[r]["context"][el] = c
                a = ea["base"][r][el] + b_acc
                ea["base"][r][el] = a; self.t[r]["gsq_context"][el] = a
                a = eab["base"][r][self.hubs] + b_accb
                eab["base"][r][self.hubs] = a; self.t[r]["gsq_cbias"][self.hubs] = a
                c = eb["base"][r][self.hubs] + b_bias / np.fmax(b_cnt, F(1))
                eb["base"][r][self.hubs] = c; self.t[r]["cbias"][self.hubs] = c


# ---- designed tables --------------------------------------------------------------------------------------------------------------
# The first delta of an "edge" element is exactly one of these words: the test zeroes the edge rows before ge_sync is created, so
# the base is 0 and table - base is the table.  (class, word)
EDGE_WORDS = (
    ("tie_even_pos", 0x3F808000), ("tie_odd_pos", 0x3F818000), ("tie_even_neg", 0xBF808000), ("tie_odd_neg", 0xBF818000),
    ("low_7fff", 0x3F807FFF), ("low_8001", 0x3F808001), ("carry_into_exponent", 0x3F7FFFFF),
    ("plus_zero", 0x00000000), ("minus_zero", 0x80000000), ("smallest_normal", 0x00800000),
    ("subnormal_tie_even", 0x00008000), ("subnormal_tie_odd", 0x00018000), ("tie_odd_pos_small", 0x3A818000),
    ("huge", 0x44800000), ("below_ulp", 0x33800000),            # 1024 beside 2^-24: the second vanishes in the sum of the two
    ("plain", 0x3DCCCCCD),
)
EDGE = np.array([w for _, w in EDGE_WORDS], np.uint32).view(F)
MEAN_EDGE = 8                                                    # the last elements of cBias carry the mean rule's designed moves


def edge_rows(D, world):
    """Rows the edge block needs: one period of (world one-mover sections, one all-movers section, one section nobody moves)."""
    return -(-(world + 2) * len(EDGE) // D)


def edge_block(V, D, world, rank):
    """Rank `rank`'s designed first moves of a [V x D] table: (first flat element of the block, values).  The block is the table's
    LAST edge_rows() rows (so the last partial group of every kernel carries designed words).  Element j of the block, by
    j mod (world + 2) * n:  section s < world: word j mod n on rank s alone;  section world: word (j + rank) mod n on every rank;
    the last section: nobody."""
    n, R = len(EDGE), edge_rows(D, world)
    j = np.arange(R * D)
    sec, k = (j // n) % (world + 2), j % n
    vals = np.zeros(R * D, F)
    one = sec == rank
    vals[one] = EDGE[k[one]]
    everyone = sec == world
    vals[everyone] = EDGE[(k[everyone] + rank) % n]
    return (V - R) * D, vals


def mean_edge(world, rank):
    """cBias, last MEAN_EDGE elements (base 0): nobody | rank 0 alone | all ranks | +x on rank 0, -x on rank 1 (sum 0, count 2) |
    -0.0 on rank 0 and x on the last rank (count 1) | rank 0 alone, a subnormal | all ranks, the same x | nobody."""
    v = np.zeros(MEAN_EDGE, F)
    last = world - 1
    v[1] = 0.375 if rank == 0 else 0.0
    v[2] = F(0.1) * F(rank + 1)
    v[3] = {0: 0.7, 1: -0.7}.get(rank, 0.0)
    v[4] = -0.0 if rank == 0 else (0.3 if rank == last else 0.0)
    v[5] = np.array([0x00000003], np.uint32).view(F)[0] if rank == 0 else 0.0
    v[6] = 0.2
    return v


def zero_edges(tables, V, D, world):
    """What a test does to every rank's tables BEFORE ge_sync is created: the edge rows of both row tables and the designed elements of
    cBias become 0 (in place)."""
    first = (V - edge_rows(D, world)) * D
    tables["context"][first:] = 0
    tables["gsq_context"][first:] = 0
    tables["cbias"][V - MEAN_EDGE:] = 0
    return tables


def moves(tables, V, D, world, rank, step, density=0.3, seed=7, designed=True, keep=None, nan_at=None):
    """Rank `rank`'s tables after its local "pass" before step `step`: sparse random moves of 1e-2 (an element is moved by all, by
    some or by no rank) on the rows of `keep` (bool [V]; None: all), and -- designed -- in step 0 the designed words on top of the
    zeroed edge elements; step 1 leaves the edge block of gradSqContext alone, whose first take is the second call.  nan_at: a flat
    element of the context table that becomes, on rank 0 in step 0, a NaN whose payload sits in the low half only (the other ranks
    get theirs over the wire).  Returns new arrays."""
    rng = np.random.default_rng([seed, rank, step])
    first, vals = edge_block(V, D, world, rank)
    out = {}
    for k in NAMES:
        cur = np.asarray(tables[k], F)
        mv = rng.standard_normal(cur.size, dtype=F) * F(0.01) * (rng.random(cur.size, dtype=F) < F(density))
        if keep is not None:
            mv = (mv.reshape(V, -1) * np.asarray(keep, bool)[:, None]).reshape(-1).astype(F)
        if designed and step == 1 and k == "gsq_context":
            mv[first:] = 0
        with np.errstate(invalid="ignore"):
            out[k] = np.where(mv != 0, cur + mv, cur)            # (an unmoved element keeps its word: -0.0 + 0.0 would be +0.0)
    if designed and step == 0:
        out["context"][first:] = vals
        out["gsq_context"][first:] = vals
        out["cbias"][V - MEAN_EDGE:] = mean_edge(world, rank)
    if nan_at is not None and step == 0 and rank == 0:
        out["context"][nan_at] = np.array([0x7F800001], np.uint32).view(F)[0]
    return out


# The call sequence of the GPU tests (accum_every = 2: the lazy entries are taken on calls 2, 4, 6 and by replicate, so a take of theirs
# has land-only and take-only neighbours; four turns follow the first take).  A "pass" of moves precedes every step.
STEPS = ("turn", "turn", "sync", "turn", "finish+begin", "sync", "replicate")


def run_step(x, step):
    """One step on anything with ge_sync's calls (the model, or a ContextSync); yields after every exchange call."""
    if step == "finish+begin":
        x.finish(); yield "finish"
        x.begin(); yield "begin"
    else:
        getattr(x, step)(); yield step


# ge_sync_epoch's order around the hub rows: their small exchange twice with moves of every row in between, then the large exchange,
# which finds only the other rows moved.
HUB_STEPS = ("hub_exchange", "hub_exchange", "sync", "replicate")


def play(model, V, D, steps=STEPS, designed=True, nan_at=None, seed=7):
    """The whole run of a test on the model: before every step each rank's pass (moves), then the step.  Yields, after every exchange
    call, (the call's name, what set_state wrote before it -- per rank, or None for the second call of a step --, every rank's
    tables after it)."""
    hub = np.zeros(V, bool); hub[model.hubs] = True
    for i, step in enumerate(steps):
        keep = ~hub if (steps is HUB_STEPS and i >= 2) else None
        sets = []
        for r in range(model.world):
            new = moves(model.tables(r), V, D, model.world, r, i, seed=seed, designed=designed, keep=keep, nan_at=nan_at)
            for k in NAMES:
                model.set(r, k, new[k])
            sets.append(new)
        for n, call in enumerate(run_step(model, step)):
            yield call, (sets if n == 0 else None), [model.tables(r) for r in range(model.world)]


def differing(a, b, nan_at=None):
    """Flat indices where two fp32 arrays differ as uint32 words (nan_at: an element that only has to be a NaN in both)."""
    a, b = np.ascontiguousarray(a, F).reshape(-1), np.ascontiguousarray(b, F).reshape(-1)
    bad = a.view(np.uint32) != b.view(np.uint32)
    if nan_at is not None and np.isnan(a[nan_at]) and np.isnan(b[nan_at]):
        bad[nan_at] = False
    return np.nonzero(bad)[0]


# The small cases of the GPU file (rows' dtype, dim, layout flags, world, wire), V = V_SMALL rows each: the smallest shapes that reach
#   k_sync_turn_flat4<W16> over fat rows (dim 32: row stride 36; dim 200: 204), over records (separate_tables) and over plain rows whose
#   stride is the dim (256);  the group's fp32 sum in rank order with three ranks;  the generic k_sync_turn<W16> (a dim that is no
#   multiple of 4);  k_exchange_turn_bf16 and the seed sequence through ge_sync (bf16 rows, three groups of four per row and 75).
V_SMALL = 300
SMALL_CASES = (("f32", 32, (), 2, "bf16"), ("f32", 32, (), 3, "bf16"), ("f32", 32, (), 3, "f32"),
               ("f32", 200, (), 2, "bf16"), ("f32", 200, ("separate_tables",), 2, "bf16"), ("f32", 256, (), 2, "bf16"),
               ("f32", 63, (), 2, "bf16"), ("f32", 126, (), 2, "bf16"),
               ("bf16", 32, (), 2, "bf16"), ("bf16", 300, (), 2, "bf16"))


def case_id(case):
    dtype, D, layout, world, wire = case
    return "%s-D%d%s-w%d-%s" % (dtype, D, "".join("-" + l for l in layout), world, wire)
