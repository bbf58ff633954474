"""The cases of the output collector's probe (tests/emu/out_runs_probe.hip), shared by tests/test_out_runs_cpu.py and
tests/test_gpu_out_runs.py: scripts of the pushes that the contract of tests/out_runs_restatement.py allows, laid onto
trips the way the kernels make them.  The scheduler mirrors the collector's count -- what a flush leaves a lane is
flush_wave's "what the lane keeps" -- because the contract needs it: a 15- or 16-element push only where the guard
allows it, the next chunk only in a trip that finds the collector empty.  It mirrors nothing else; what the arrays must
hold comes from the restatement, which knows neither trips nor flushes.

all_cases() -> the list of cases; write_case() -> the probe's case file; check_case() compares the probe's four result
files of a case with the restatement and with the properties the case was built for."""
import functools
import os
import random
import subprocess

import numpy as np

import out_runs_restatement as orr

ALL = 0xFFFFFFFF
BLOCK = 64                 # elements per block (OutRuns::kBlock)
PERIOD = 4                 # trips between flushes
CAPACITY = 96
GUARD = 96                 # the constant of the 16-element push's guard
LANES_PER_BLOCK = 256      # kQueryBlock
MAGIC = 0x455341434E55524F
WAVE_WORDS = 72
W_WHOLE, W_RAGGED, W_MAX_EMIT, W_CANARY, W_FLUSHES, W_MIXED = 65, 66, 67, 68, 69, 70
IDLE_RECORD = (1 << 8, 0, 0, 0, 0, 0, 0, 0)
SWEEP_LENGTHS = tuple(range(1, 10)) + (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193)


class Lane:
    """One lane's chunks, its policy (what to push in a trip) and the scheduler's mirror of its state."""

    def __init__(self, chunks=(), policy=None):
        self.chunks = [(int(a), int(n)) for a, n in chunks]
        assert all(n > 0 for _, n in self.chunks)
        self.policy = policy
        self.pushes = [[] for _ in self.chunks]     # per chunk: (n, l_new, keep, keep1, ids, ids2), for the restatement
        self.records = []                           # per trip, for the probe
        self.ci = 0
        self.done = not self.chunks
        self.rem = self.chunks[0][1] if self.chunks else 0
        self.cnt = 0                                # the collector's count
        self.L = 0                                  # the value of the lane's element 0
        self.max_cnt = 0
        self.guard, self.log = GUARD, {"taken": set(), "refused": set()}     # schedule() sets both

    def gl(self):
        return self.chunks[self.ci][0] + self.rem

    def may_take_16(self, ph, up16, n=16):
        """The guard of fat2_query.hip's match tail; whoever asks takes the push when it says yes."""
        if not up16 or self.rem < n:
            return False
        allowed = self.cnt + 16 + 8 * (3 - ph) <= self.guard
        self.log["taken" if allowed else "refused"].add((ph, self.cnt))
        return allowed

    def push(self, action, ph, up16, rng):
        kind, arg, new_read = action
        if new_read:
            self.L = 0
        keep = keep1 = ALL
        if kind == "cont":
            n, l_new = arg, self.L + arg
        elif kind == "absent":
            n, l_new = arg, arg - 1
            assert 1 <= n <= 8
        elif kind == "scan":
            n, l_new = 1, 0
        elif kind == "entry2":
            n, l_new, keep = 2, 1, ALL if arg else 0
        elif kind == "deep":
            n, l_new = 3, 2 if arg else 1
            keep1 = ALL if arg else 0
        else:
            raise ValueError(kind)
        assert n <= self.rem, "a push stays inside its chunk"
        if n > 8:
            assert kind == "cont" and n in (15, 16) and up16
            assert self.cnt + 16 + 8 * (3 - ph) <= self.guard, "the guard of the 16-element push"
        ids, ids2 = rng.getrandbits(64), rng.getrandbits(64)          # the bytes from byte n on are garbage
        if n:
            self.L = l_new if keep else 0
        self.rem -= n
        self.cnt += n
        self.max_cnt = max(self.max_cnt, self.cnt)
        self.pushes[self.ci].append((n, l_new, keep, keep1, ids, ids2))
        self.records.append((n, l_new, keep, keep1, ids & ALL, ids >> 32, ids2 & ALL, ids2 >> 32))

    def flush(self):
        """The count's side of flush_wave -> (emits an item A, it is a whole block, emits an item B)."""
        below = -self.gl() % BLOCK
        final = self.rem == 0
        has_a = below < self.cnt
        has_b = final and min(below, self.cnt) != 0
        whole = has_a and self.cnt - below == BLOCK
        assert not has_a or self.cnt - below <= BLOCK
        if has_a or has_b:
            self.cnt = 0 if final else below
        return has_a, whole, has_b

    def finished(self):
        return self.done or (self.rem == 0 and self.cnt == 0 and self.ci == len(self.chunks) - 1)


def schedule(lanes, up16, seed, guard=GUARD):
    """Plays every lane's policy trip by trip -> (n_trips, what the probe's wave words must say, the guard's log)."""
    assert len(lanes) % LANES_PER_BLOCK == 0
    rng = random.Random(seed)
    n_waves = len(lanes) // 64
    waves = np.zeros((n_waves, WAVE_WORDS), np.uint32)
    waves[:, W_CANARY] = 1
    log = {"taken": set(), "refused": set()}
    for ln in lanes:
        ln.guard, ln.log = guard, log
    live = [(i, ln) for i, ln in enumerate(lanes) if not ln.done]
    trip = 0
    while True:
        ph = trip % PERIOD
        emit = np.zeros(n_waves, np.int64)
        kinds = np.zeros((n_waves, 3), np.int64)
        for i, ln in live:
            if ln.done:
                continue
            if ln.rem == 0 and ln.cnt == 0:                       # the flush has taken everything: the next chunk
                ln.ci += 1
                if ln.ci == len(ln.chunks):
                    ln.ci -= 1
                    ln.done = True
                    continue
                ln.rem, ln.L = ln.chunks[ln.ci][1], 0
            action = ln.policy(ln, ph, up16, rng) if ln.rem else None
            if action is None:
                ln.records.append(IDLE_RECORD)
            else:
                ln.push(action, ph, up16, rng)
            if ph == PERIOD - 1:
                has_a, whole, has_b = ln.flush()
                emit[i // 64] += has_a or has_b
                kinds[i // 64] += (whole, has_a and not whole, has_b)
        if ph == PERIOD - 1:
            for w in range(n_waves):
                waves[w, emit[w]] += 1
                waves[w, W_WHOLE] += kinds[w, 0]
                waves[w, W_RAGGED] += kinds[w, 1] + kinds[w, 2]
                waves[w, W_MAX_EMIT] = max(waves[w, W_MAX_EMIT], emit[w])
                waves[w, W_FLUSHES] += 1
                waves[w, W_MIXED] += bool(kinds[w, 0] and kinds[w, 1] and kinds[w, 2])
            live = [(i, ln) for i, ln in live if not ln.finished()]
            if not live:
                return trip + 1, waves, log
        trip += 1
        assert trip < 100000


# ---- policies: (lane, phase, up16, rng) -> None (idle) or (kind, argument, new read)

def greedy(n16=(16,), plain="most"):
    """A 15- or 16-element continuation in every trip the guard allows, else a plain continuation: the most the chunk
    has left up to 8, or (plain="any") 0 .. 8."""
    def policy(ln, ph, up16, rng):
        n = rng.choice(n16)
        if ln.may_take_16(ph, up16, n):
            return ("cont", n, False)
        most = min(8, ln.rem)
        return ("cont", most if plain == "most" else rng.randint(0, most), False)
    return policy


def plain8(ln, ph, up16, rng):
    return ("cont", min(8, ln.rem), False)


def mixed(p_idle=0.08, p_new=1 / 40):
    """Push kinds drawn from the contract."""
    def policy(ln, ph, up16, rng):
        if rng.random() < p_idle:
            return None
        new_read = rng.random() < p_new
        r = rng.random()
        if r < 0.25 and ln.may_take_16(ph, up16, 15):
            return ("cont", 16 if ln.rem >= 16 and rng.random() < 0.6 else 15, new_read)
        if r < 0.55:
            return ("cont", rng.randint(0, min(8, ln.rem)), new_read)
        if r < 0.70:
            return ("absent", rng.randint(1, min(8, ln.rem)), new_read)
        if r < 0.80 or ln.rem < 2:
            return ("scan", 1, new_read)
        if r < 0.90 or ln.rem < 3:
            return ("entry2", rng.random() < 0.5, new_read)
        return ("deep", rng.random() < 0.5, new_read)
    return policy


def scripted(actions, then=plain8):
    """The given actions, one per trip the lane is live in (None: idle), then another policy."""
    todo = list(actions)

    def policy(ln, ph, up16, rng):
        if todo:
            return todo.pop(0)
        return then(ln, ph, up16, rng)
    return policy


class Layout:
    """Chunk addresses in ascending order with guard elements in between."""

    def __init__(self):
        self.cur = BLOCK

    def place(self, length, residue=None, gap=3):
        a = self.cur + gap
        if residue is not None:
            a += (residue - a) % BLOCK
        self.cur = a + length
        return a

    def n_out(self):
        return self.cur + BLOCK


def pad_lanes(lanes):
    return lanes + [Lane() for _ in range(-len(lanes) % LANES_PER_BLOCK)]


def make_case(name, lanes, n_out, up16, seed, bias=0, guard=GUARD):
    lanes = pad_lanes(lanes)
    n_trips, waves, log = schedule(lanes, up16, seed, guard)
    return {"name": name, "lanes": lanes, "n_out": n_out, "up16": up16, "bias": bias, "n_trips": n_trips, "waves": waves, "log": log}


# ---- the cases

def alignment_case(up16):
    """Every chunk base residue mod 64 with every length of SWEEP_LENGTHS: heads and tails at every residue of a PML
    piece (8) and of a col-id piece (16), chunks inside one block, ending at one, spanning up to four."""
    rng = random.Random(11)
    shapes = [(res, n) for res in range(BLOCK) for n in SWEEP_LENGTHS]
    rng.shuffle(shapes)
    lay = Layout()
    per_lane = [[] for _ in range(LANES_PER_BLOCK)]
    for k, (res, n) in enumerate(shapes):
        per_lane[k % LANES_PER_BLOCK].append((lay.place(n, res, gap=rng.randint(1, 9)), n))
    lanes = [Lane(ch, mixed() if i % 3 else greedy((15, 16), "any")) for i, ch in enumerate(per_lane)]
    case = make_case(f"alignment{16 if up16 else 8}", lanes, lay.n_out(), up16, 12)
    heads = {(a % BLOCK, n) for ln in lanes for a, n in ln.chunks}
    assert heads == set(shapes) and {(a + n) % 16 for a, n in heads} == set(range(16))
    return case


def emitting_case(up16):
    """Flushes in which exactly 1, 31, 32, 33 and 64 lanes of a wave emit, a wave in which nobody emits, a wave without
    chunks, waves that mix whole blocks with ragged items A and B, a final flush that finds exactly one whole block."""
    rng = random.Random(21)
    lay = Layout()
    lanes = []

    def wave(make):
        made = [make(k) for k in range(64)]
        rng.shuffle(made)                     # which lanes of the wave: by chance, a lane's rank is not its number
        lanes.extend(made)

    def short_chunks(count):
        return [(lay.place(n, rng.randrange(BLOCK)), n) for n in (rng.randint(1, 32) for _ in range(count))]

    # waves 0 - 4: three flushes with exactly E emitting lanes (every chunk of up to 32 elements is reported within
    # its period, 8 a trip)
    for emitters in (1, 31, 32, 33, 64):
        wave(lambda k: Lane(short_chunks(3), plain8) if k < emitters else Lane())
    # wave 5: nobody emits in the first flush (32 elements that reach no block boundary, 8 still to come)
    wave(lambda k: Lane([(lay.place(40, 10), 40)], plain8))
    # wave 6: no lane has a chunk
    wave(lambda k: Lane())
    # wave 7: long chunks (whole blocks in non-final flushes), chains of short ones, and everything the contract has
    wave(lambda k: Lane([(lay.place(200 + k, rng.randrange(BLOCK)), 200 + k)], greedy((15, 16))) if k < 20 else
         Lane(short_chunks(5), plain8) if k < 40 else Lane(short_chunks(4) + [(lay.place(150, k), 150)], mixed()))
    # wave 8: 64 lanes with an item A and an item B each: two passes of 32 slots, both full of items
    wave(lambda k: Lane([(lay.place(30, 64 - 11 - k % 8), 30)], plain8))
    # wave 9: a final flush that finds exactly one whole block and nothing below it (a block-aligned chunk of 64:
    # four pushes of 16, or eight of 8 with a flush in between that nobody emits in), and next to it 128 and 192
    wave(lambda k: Lane([(lay.place(64 * (1 + k % 3), 0), 64 * (1 + k % 3))], greedy()))
    # wave 10: 33 lanes with two items each: the second pass holds one lane
    wave(lambda k: Lane([(lay.place(20, 64 - 7), 20)], plain8) if k < 33 else Lane())
    # wave 11: whole blocks, ragged tops and final rests in the same flushes
    wave(lambda k: Lane([(lay.place(100 + 3 * k, rng.randrange(BLOCK)), 100 + 3 * k)], greedy((15, 16), "any")) if k % 2 else
         Lane(short_chunks(6), mixed(p_idle=0.3)))
    case = make_case(f"emitting{16 if up16 else 8}", lanes, lay.n_out(), up16, 22)
    w = case["waves"]
    for k, emitters in enumerate((1, 31, 32, 33, 64)):
        assert w[k, emitters] == 3 and w[k, W_MAX_EMIT] == emitters, (k, w[k])
    assert w[5, 0] >= 1 and w[5, 64] == 1 and w[6, 0] == w[6, W_FLUSHES] and w[6, W_MAX_EMIT] == 0
    assert w[8, 64] == 1 and w[8, W_RAGGED] == 128 and w[10, 33] == 1 and w[10, W_RAGGED] == 66
    assert w[9, W_WHOLE] == 22 * 1 + 21 * 2 + 21 * 3 and w[9, W_RAGGED] == 0, w[9]
    assert w[7, W_MIXED] >= 1 and w[11, W_MIXED] >= 1
    return case


def push_kinds(up16):
    """Every push of the contract as (kind, argument, elements)."""
    kinds = [("cont", n, n) for n in range(9)] + ([("cont", 15, 15), ("cont", 16, 16)] if up16 else [])
    kinds += [("absent", n, n) for n in range(1, 9)] + [("scan", 1, 1)]
    kinds += [("entry2", True, 2), ("entry2", False, 2), ("deep", True, 3), ("deep", False, 3)]
    return kinds


def seams_case(up16):
    """Every push kind placed with each of its elements just above a 64-element block boundary, an 8-element PML piece
    boundary and a 16-element col-id piece boundary (the boundary between elements d - 1 and d of the push, d = 0 .. n:
    below, inside at every place, above), as the first push of its chunk and after a continuation of 5, as a
    continuation of the same read and as the first push of a new read, with the chunk ending right below the push (the
    final flush takes items A and B at once) and with 70 more elements of continuation below it (a non-final flush cuts
    at the block boundary, and the value just above the cut feeds the next flush).  The push is made in every phase of
    the flush period."""
    lay = Layout()
    lanes = []
    for kind, arg, n in push_kinds(up16):
        for d in range(n + 1):
            for boundary in (0, 8, 16):
                for prefix, new_read in ((0, False), (5, False), (5, True)):
                    if new_read and kind != "cont":
                        continue                               # the other kinds say their values themselves
                    for suffix in (0, 70):
                        length = prefix + n + suffix
                        if length == 0:
                            continue                           # an empty push alone is no chunk
                        base = lay.place(length, (boundary - d - suffix) % BLOCK)
                        lead = len(lanes) % PERIOD             # the guard holds in every phase: cnt <= 5
                        acts = [None] * lead + ([("cont", prefix, False)] if prefix else []) + [(kind, arg, new_read)]
                        lanes.append(Lane([(base, length)], scripted(acts)))
                        assert (base + suffix + d) % BLOCK == boundary
    return make_case(f"seams{16 if up16 else 8}", lanes, lay.n_out(), up16, 32)


def guard_case(guard=GUARD):
    """A 15- or 16-element push in every trip the guard allows: chunk tops at every residue mod 64, so that a flush
    leaves every count 0 .. 63, plain pushes of 8 or of 0 .. 8 in the trips it refuses.  The largest count is exactly 96,
    and in every phase the guard is met with the largest count it allows and with that count plus one."""
    rng = random.Random(41)
    lay = Layout()
    lanes = []
    for k in range(LANES_PER_BLOCK):
        n = 300 + rng.randint(0, 120)
        policy = (greedy((16,)), greedy((15,)), greedy((15, 16), "any"), greedy((16,), "any"))[k // BLOCK]
        lanes.append(Lane([(lay.place(n, (k - n) % BLOCK), n)], policy))
    case = make_case("guard16", lanes, lay.n_out(), True, 42, guard=guard)
    if guard == GUARD:
        assert max(ln.max_cnt for ln in case["lanes"]) == CAPACITY
        for ph in range(PERIOD):
            limit = GUARD - 16 - 8 * (3 - ph)
            assert (ph, limit) in case["log"]["taken"] and (ph, limit + 1) in case["log"]["refused"], (ph, limit)
            assert all(c <= limit for p, c in case["log"]["taken"] if p == ph)
    return case


def long_case():
    """One lane reports a single all-match read of 65 535 bases (values 1 .. 65 535 from the top down, the largest a
    16-bit PML holds) while the other lanes have nothing: no value wraps in the parked piece headers."""
    lay = Layout()
    lanes = [Lane() for _ in range(LANES_PER_BLOCK)]
    lanes[77] = Lane([(lay.place(65535, 13), 65535)], greedy((16,)))
    return make_case("long16", lanes, lay.n_out(), True, 52)


def random_lanes(seed, n_lanes=LANES_PER_BLOCK, bias=0):
    rng = random.Random(seed)
    counts = [rng.randint(1, 6) for _ in range(n_lanes)]
    owners = [i for i, c in enumerate(counts) for _ in range(c)]
    rng.shuffle(owners)
    lay = Layout()
    per_lane = [[] for _ in range(n_lanes)]
    for i in owners:
        n = rng.randint(91, 700) if rng.random() < 0.02 else rng.randint(1, 90)
        per_lane[i].append((bias + lay.place(n, gap=rng.randint(0, 69)), n))
    return [Lane(ch, mixed()) for ch in per_lane], lay.n_out()


def random_case(seed, up16=True):
    """256 lanes, up to 6 chunks each of 1 .. 90 elements and a few of up to 700, 0 .. 69 elements between neighbours,
    push kinds drawn from the contract, a new read on about 1 push in 40."""
    lanes, n_out = random_lanes(seed)
    return make_case(f"random{16 if up16 else 8}_{seed}", lanes, n_out, up16, seed + 1000)


def high_case(k, bias):
    """Element addresses at and above 2^32: the arrays reach the kernel lowered by `bias` elements and the chunk
    addresses are raised by as much, so an item's address needs its high dword (and carries into it)."""
    lanes, n_out = random_lanes(60 + k, bias=bias)
    assert bias % 16 == 0 and bias + n_out > 1 << 32
    return make_case(f"high16_{k}", lanes, n_out, True, 70 + k, bias=bias)


CASE_NAMES = ("alignment16", "emitting16", "seams16", "guard16", "long16", "high16_0", "high16_1", "high16_2", "random16_1", "random16_2",
              "random16_3", "random16_4", "random16_5", "alignment8", "emitting8", "seams8", "random8_6")


@functools.lru_cache(maxsize=None)
def all_cases():
    """Computed once, shared by the tests and left unchanged."""
    cases = [alignment_case(True), emitting_case(True), seams_case(True), guard_case(), long_case()]
    cases += [high_case(0, (1 << 32) + 4096), high_case(1, (1 << 32) - 2048), high_case(2, (7 << 32) + 4096)]
    cases += [random_case(seed) for seed in (1, 2, 3, 4, 5)]
    cases += [alignment_case(False), emitting_case(False), seams_case(False), random_case(6, up16=False)]
    assert tuple(c["name"] for c in cases) == CASE_NAMES
    return cases


def case_named(name):
    return all_cases()[CASE_NAMES.index(name)]


# ---- the probe's files

def run_probe(command, directory, timeout):
    """Writes every case into `directory` and runs the probe -- `command` is the program, with whatever goes in front of
    it -- over all of them in one process -> the finished process."""
    for c in all_cases():
        write_case(f"{directory}/{c['name']}.case", c)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    return subprocess.run(list(command) + [str(directory)] + list(CASE_NAMES), env=env, capture_output=True, text=True, timeout=timeout)


def write_case(path, case):
    lanes = case["lanes"]
    max_chunks = max(1, max(len(ln.chunks) for ln in lanes))
    counts = np.array([len(ln.records) for ln in lanes], np.uint64)
    lane_tab = np.zeros((len(lanes), 2), np.uint64)
    lane_tab[:, 0] = np.concatenate([[0], np.cumsum(counts)[:-1]])
    lane_tab[:, 1] = counts
    chunk_tab = np.zeros((len(lanes), max_chunks, 2), np.uint64)
    for i, ln in enumerate(lanes):
        for c, (a, n) in enumerate(ln.chunks):
            chunk_tab[i, c] = (a, n)
    records = np.array([r for ln in lanes for r in ln.records], np.uint32).reshape(-1, 8)
    header = np.array([MAGIC, len(lanes), case["n_trips"], max_chunks, case["n_out"], case["bias"], int(case["up16"]), len(records)], np.uint64)
    with open(path, "wb") as f:
        for part in (header, lane_tab, chunk_tab, records):
            f.write(part.tobytes())


@functools.lru_cache(maxsize=None)
def _expected(name):
    chunks = [(a, n, pushes) for ln in case_named(name)["lanes"] for (a, n), pushes in zip(ln.chunks, ln.pushes)]
    return orr.apply(case_named(name)["n_out"], chunks, case_named(name)["bias"])


def describe(case, at):
    """Which lane, chunk, trip and element of a push wrote output element `at`: what a failure should point at."""
    at += case["bias"]
    for i, ln in enumerate(case["lanes"]):
        for c, (a, n) in enumerate(ln.chunks):
            if a <= at < a + n:
                rem, trip = n, -1
                pushing = [t for t, r in enumerate(ln.records) if not r[0] >> 8]
                before = sum(len(p) for p in ln.pushes[:c])
                for k, push in enumerate(ln.pushes[c]):
                    if a + rem - push[0] <= at:
                        trip = pushing[before + k]
                        return (f"lane {i} (wave {i // 64}, lane {i % 64}), chunk {c} = [{a}, {a + n}), trip {trip}, "
                                f"element {at - (a + rem - push[0])} of push (n, l_new, keep, keep1) = {push[:4]}")
                    rem -= push[0]
    return "outside every chunk (a guard element)"


def check_case(case, directory):
    """The probe's result files of a case against the restatement and the scheduler's mirror."""
    name = case["name"]
    lanes = np.fromfile(f"{directory}/{name}.lanes", np.uint32).reshape(-1, 4)
    waves = np.fromfile(f"{directory}/{name}.waves", np.uint32).reshape(-1, WAVE_WORDS)
    assert len(lanes) == len(case["lanes"])
    assert (lanes[:, 0] <= CAPACITY).all(), f"{name}: a script asks the collector for {lanes[:, 0].max()} elements, it holds {CAPACITY}"
    assert (lanes[:, 3] == 0).all(), f"{name}: the probe refused a push of lanes {np.flatnonzero(lanes[:, 3])[:8]}"
    want_pml, want_cid = _expected(name)
    for ext, want in ((".pml", want_pml), (".cid", want_cid)):
        got = np.fromfile(f"{directory}/{name}{ext}", want.dtype)
        assert got.shape == want.shape, name
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"{name}{ext}: {bad.size} elements differ, the first at {bad[0]}: {got[bad[0]]} instead of "
                               f"{want[bad[0]]}; {describe(case, int(bad[0]))}")
    assert (lanes[:, 0] == [ln.max_cnt for ln in case["lanes"]]).all(), f"{name}: largest counts differ from the scheduler's"
    assert (lanes[:, 1] == 0).all() and (lanes[:, 2] == 1).all(), f"{name}: lanes {np.flatnonzero(lanes[:, 2] != 1)[:8]} have not finished"
    assert (waves[:, W_CANARY] == 1).all(), f"{name}: canary words behind the flush's LDS area overwritten"
    assert (waves[:, :71] == case["waves"][:, :71]).all(), f"{name}: flush counts differ from the scheduler's"
    return lanes, waves
