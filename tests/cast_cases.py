"""The frames that hold cast detection (detect_image_type, six_stadigy.py:292-302) on the device to NumPy's sequential float32
mean at every path of its closed-form restatement (k_entry.hip), and the analyser that says which paths a frame reaches.
NumPy and the oracle only, seeded, no GPU.  tests/test_cast_cases.py asserts on the CPU that every frame is what it claims to
be; tests/test_gpu_cast.py compares the device with NumPy on them.

The device never adds the pixels one by one.  Inside one binade [2^e, 2^(e+1)) of the accumulator a pixel advances it by a whole
number of ulps, so a 16384-pixel chunk advances it by a number that follows from the chunk's histogram (k_chunk_hist,
k_chunk_hist_quad, k_chunk_ulps).  k_cast_resolve walks the chunks 64 at a time and "drills" a chunk -- 1024 threads x 16
pixels, the same scan again -- only where an EVENT sits: the accumulator leaves its binade (a crossing), or a pixel's
x / ulp has fraction exactly 1/2 (a tie: round-half-even then depends on the parity of the running sum).  Sequential adds
happen only in the 16 pixels of the thread that holds the event, and in the first 1024 pixels ("head") of a chunk that starts
with an accumulator below 0.25.  `events` finds the events of a stream from NumPy's own accumulation and restates the
kernel's STRUCTURE (which chunk is drilled, from which walk lane, which thread and pixel holds the event), not its
arithmetic.

A zero pixel adds nothing to a float32 sum, so `zeros + content + zeros` moves an event to any chunk, thread and pixel at no
cost: the cases are sparse streams, one per channel, not large dense frames.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

CHUNK = 16384         # k_entry.hip: kChunkPx, pixels per histogram chunk
DRILL_THREADS = 1024  # k_entry.hip: kResolveThreads, threads of a drill ...
DRILL_PER = 16        # k_entry.hip: kResolvePer, ... and the pixels each of them holds (1024 x 16 = one chunk)
WALK = 64             # k_entry.hip: kWave lanes of wavefront 0 in k_cast_resolve, chunks per prefix scan of the walk
HEAD = 1024           # k_entry.hip: kResolveHead, pixels added one by one when a drill starts below 0.25
SMALL = np.float32(0.25)  # common.h: 2^kCastBinadeMin, the smallest accumulator handled in closed form
assert DRILL_THREADS * DRILL_PER == CHUNK

F32 = np.float32
ODD_W = 1001  # frames of this width are unaligned from the second row on and leave a ragged four-pixel tail
EVEN_W = 1000  # a multiple of 8


def binade(v):
    """Exponent field of float32 values, as the kernels read it: floor(log2 v) for normal v, -127 for 0."""
    return (np.ascontiguousarray(v, dtype=F32).view(np.uint32) >> 23).astype(np.int32) - 127


def tie_binade(k):
    """The one binade e in which byte value k ties (float32(k) / 255 over ulp_e has fraction 1/2), or None.
    x = M * 2^E with an odd M: x / 2^(e-23) = n + 1/2 pins e = E + 24."""
    if k == 0:
        return None
    m, ex = np.frexp(np.float64(F32(k) / F32(255)))  # x = m * 2^ex, 0.5 <= m < 1
    M = int(m * (1 << 24))  # 24 significant bits
    E = int(ex) - 24
    while M % 2 == 0:
        M //= 2
        E += 1
    return E + 24


class Report(NamedTuple):
    npx: int
    total: np.float32        # the sequential float32 sum of the stream
    cross: np.ndarray        # pixel indices where the accumulator's exponent changes (previous sum >= 0.25)
    landing: np.ndarray      # per crossing: the new sum is a power of two exactly
    tie: np.ndarray          # pixel indices of round-half-even ties (previous sum >= 0.25, pixel > 0)
    tie_up: np.ndarray       # per tie: rounded up (the running sum was odd) or down
    tie_in_head: np.ndarray  # per tie: inside the sequential head of its drill
    drilled: np.ndarray      # chunk indices the kernel drills: start below 0.25, or an event inside
    headed: np.ndarray       # per drilled chunk: starts below 0.25 (no walk leads to it, its first 1024 pixels are the head)
    lane: np.ndarray         # per drilled chunk: (c - start) % 64, start = the chunk behind the previous drill; -1 if headed
    trip: np.ndarray         # per drilled chunk: (c - start) // 64; -1 if headed
    ncross: np.ndarray       # per drilled chunk: crossings inside
    ntie: np.ndarray         # per drilled chunk: ties inside
    gain: np.ndarray         # per drilled chunk: binades gained across it (everything below 0.25 counts as one binade)
    walked_next: np.ndarray  # per drilled chunk: the next chunk exists and is not drilled
    left_after: int          # chunks behind the last drill (the whole frame if nothing is drilled)

    @property
    def nchunk(self):
        return -(-self.npx // CHUNK)

    @property
    def mean(self):
        """NumPy's _mean: the float32 sum divided in float64, rounded to float32."""
        return F32(np.float64(self.total) / np.float64(self.npx))

    def where(self, p):
        """(chunk, thread, pixel in thread) of pixel index p (arrays allowed)."""
        p = np.asarray(p)
        return p // CHUNK, (p % CHUNK) // DRILL_PER, p % DRILL_PER


def events(channel_u8) -> Report:
    u8 = np.ascontiguousarray(channel_u8, dtype=np.uint8).ravel()
    n = u8.size
    x = u8.astype(F32) / F32(255)
    acc = np.add.accumulate(x, dtype=F32)
    prev = np.empty_like(acc)
    prev[0] = 0
    prev[1:] = acc[:-1]
    live = (prev >= SMALL) & (u8 > 0)
    idx = np.flatnonzero(live)  # only these pixels can hold an event
    pv, av, xv = prev[idx], acc[idx], x[idx]
    crossed = binade(av) != binade(pv)
    cross = idx[crossed]
    m, _ = np.frexp(av[crossed])
    landing = m == 0.5
    q = xv.astype(np.float64) / np.spacing(pv).astype(np.float64)
    tied = (q - np.floor(q)) == 0.5
    tie = idx[tied]
    tie_up = (av[tied].astype(np.float64) - pv[tied].astype(np.float64)) > xv[tied].astype(np.float64)

    nchunk = -(-n // CHUNK)
    start_sum = prev[::CHUNK]
    end_sum = acc[np.minimum(np.arange(1, nchunk + 1) * CHUNK, n) - 1]
    headed_all = start_sum < SMALL
    ncross_all = np.bincount(cross // CHUNK, minlength=nchunk)
    ntie_all = np.bincount(tie // CHUNK, minlength=nchunk)
    is_drilled = headed_all | (ncross_all > 0) | (ntie_all > 0)
    drilled = np.flatnonzero(is_drilled)
    headed = headed_all[drilled]
    start = np.concatenate([[0], drilled[:-1] + 1])
    lane = np.where(headed, -1, (drilled - start) % WALK)
    trip = np.where(headed, -1, (drilled - start) // WALK)
    floor_e = binade(SMALL) - 1
    gain = np.maximum(binade(end_sum[drilled]), floor_e) - np.maximum(binade(start_sum[drilled]), floor_e)
    nxt = drilled + 1
    walked_next = (nxt < nchunk) & ~is_drilled[np.minimum(nxt, nchunk - 1)]
    tie_in_head = headed_all[tie // CHUNK] & (tie % CHUNK < HEAD)
    left = nchunk - (int(drilled[-1]) + 1) if drilled.size else nchunk
    return Report(n, acc[-1], cross, landing, tie, tie_up, tie_in_head, drilled, headed, lane, trip, ncross_all[drilled],
                  ntie_all[drilled], gain, walked_next, left)


# ---------------------------------------------------------------------------------------------------------------- cases
class Case(NamedTuple):
    name: str
    group: int      # the case number of the list in the module docstring of tests/test_cast_cases.py
    u8: np.ndarray  # (H, W, 3), read-only


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def frame_of(streams, W, npx=None):
    """Three flat byte streams -> (H, W, 3): padded with zeros (or cut: the caller's streams end in zeros then) to H * W pixels,
    H * W = npx, or the smallest multiple of W that holds the longest stream."""
    longest = max(len(s) for s in streams)
    if npx is None:
        npx = -(-longest // W) * W
    assert npx % W == 0, (npx, W)
    out = np.zeros((npx, 3), np.uint8)
    for c, s in enumerate(streams):
        s = np.asarray(s, np.uint8)
        assert not s[npx:].any(), "content cut off"
        out[: min(len(s), npx), c] = s[:npx]
    out = out.reshape(npx // W, W, 3)
    out.setflags(write=False)
    return out


def rows_for_chunks(nchunk, W):
    """H such that H * W pixels make exactly `nchunk` chunks (the last one ragged unless W divides it)."""
    H = nchunk * CHUNK // W
    assert -(-H * W // CHUNK) == nchunk
    return H


class Stream:
    """A sparse stream of bytes under construction: black, with content put at stated pixel positions."""

    def __init__(self, n):
        self.v = np.zeros(n, np.uint8)

    def put(self, pos, values):
        values = np.atleast_1d(np.asarray(values, np.uint8))
        assert not self.v[pos : pos + len(values)].any(), "overlapping content"
        self.v[pos : pos + len(values)] = values

    def whites_ending_at(self, pos, count):
        """`count` pixels of 255 in one run whose last pixel is `pos`."""
        self.put(pos - count + 1, np.full(count, 255, np.uint8))


def at(chunk, thread=0, pixel=0):
    return chunk * CHUNK + thread * DRILL_PER + pixel


# 1 ---- walk lanes.  All-255 content: the sum is the count, it lands on 2^k at the 2^k-th pixel, and 255 ties in binade 24 only
def _walk(nchunk, W, plans):
    """plans: per channel a list of chunk indices; chunk 0 is headed (3 pixels -> sum 3), then every listed chunk holds the
    pixels that take the sum to the next power of two (a crossing there and nowhere else)."""
    streams = []
    for plan in plans:
        s = Stream(nchunk * CHUNK)
        s.whites_ending_at(at(0, 400, 2), 3)
        have = 3
        for c in plan:
            need = (1 << have.bit_length()) - have
            s.whites_ending_at(at(c, 300 + c % 7, 9), need)
            have += need
        streams.append(s.v)
    return frame_of(streams, W, rows_for_chunks(nchunk, W) * W)


def walk_a():
    # 134 chunks.  R: lanes 0, 1, 63, then 64 clean chunks (trip 1, lane 0), 1 chunk left.  G: 64 left.  B: 65 left.
    return _walk(134, ODD_W, [[1, 3, 67, 132], [2, 69], [68]])


def walk_b():
    # 70 chunks, W % 8 == 0.  R: 63 left.  G: lane 0 twice, 64 left.  B: lane 63 from the head's chunk on, 1 left.
    return _walk(70, EVEN_W, [[6], [1, 2, 5], [4, 68]])


# 2 ---- drill positions
def drill_positions():
    n = 6 * CHUNK
    r = Stream(n)  # starts at 3 behind chunk 0; crossings at (thread, pixel) = (0, 0), (63, 15), (64, 0), (1023, 15)
    r.whites_ending_at(at(0, 400, 2), 3)
    r.whites_ending_at(at(1, 0, 0), 1)
    r.whites_ending_at(at(2, 63, 15), 4)
    r.whites_ending_at(at(3, 64, 0), 8)
    r.whites_ending_at(at(4, 1023, 15), 16)
    g = Stream(n)  # a headed chunk whose head takes the sum to 1: the crossing to 2 sits in thread 64, the first behind the head
    g.put(at(0, 0, 10), 255)
    g.put(at(0, 64, 5), 255)
    g.whites_ending_at(at(2, 500, 7), 6)   # 3, 4 (crossing at pixel 3), 5, 6, 7, 8 (crossing at pixel 7): two in one thread
    g.whites_ending_at(at(2, 500, 15), 8)  # ... and the third, at 16, in its last pixel
    b = Stream(n)  # a headed chunk with an empty head: 1, 2 (crossing), 3, 4 (crossing) inside thread 64
    b.whites_ending_at(at(1, 64, 9), 4)
    return frame_of([r.v, g.v, b.v], ODD_W, rows_for_chunks(6, ODD_W) * ODD_W)


# 3 ---- several binades in one chunk
def _dim(seed, zeros, n):
    rng = np.random.default_rng([3, seed])
    return np.concatenate([np.zeros(zeros, np.uint8), rng.integers(0, 40, n, dtype=np.uint8)])


def several_binades():
    """R: dim dense noise behind 21384 zeros: its first chunk is headed and crosses many binades, the next ones 2, 1, 0.
    G: the same kind of content behind a lit start (no head): the dense chunks are reached by the walk.
    B: sparse tie-rich pixels (case 5's content) up to the first chunk that is drilled for a tie alone, black behind it: a
    drilled chunk that gains no binade, followed by a walked one."""
    r = _dim(1, 21384, 7 * CHUNK)
    g = _dim(2, 21384, 7 * CHUNK)
    g[100:103] = 255
    b = _tie_stream(1, 9 * CHUNK, 1500, 300, 8 * CHUNK)
    rep = events(b)
    only = rep.drilled[(rep.ncross == 0) & (rep.ntie > 0) & ~rep.headed]
    b[(int(only[0]) + 1) * CHUNK :] = 0
    return frame_of([r, g, b], ODD_W, rows_for_chunks(9, ODD_W) * ODD_W)


# 4 ---- exact landings
def landings_128():
    out = np.full((128, 128, 3), 255, np.uint8)
    out.setflags(write=False)
    return out


def landings_shifted():
    n = 5 * CHUNK
    streams = []
    for z in (5, 1029, 16384 + 7):  # behind z zeros the sum lands on 2^k at pixel z + 2^k - 1
        s = np.zeros(n, np.uint8)
        s[z : z + 40000] = 255
        streams.append(s)
    return frame_of(streams, ODD_W, rows_for_chunks(5, ODD_W) * ODD_W)


# 5 ---- ties past the head
TIE_RICH = list(range(135, 248, 8)) + [191, 159, 223]  # the values that tie in binades 3 - 6; 191 (6), 159 and 223 (5) twice


def _tie_stream(seed, n, first, count, span):
    """`count` pixels of the tie-rich values scattered over [first, first + span) of a stream of n zeros."""
    rng = np.random.default_rng([5, seed])
    s = np.zeros(n, np.uint8)
    pos = first + np.sort(rng.choice(span, count, replace=False))
    s[pos] = rng.choice(np.array(TIE_RICH, np.uint8), count)
    return s


def ties():
    n = 21 * CHUNK
    streams = [_tie_stream(seed, n, 1500, 600, 20 * CHUNK) for seed in (1, 2, 3)]
    return frame_of(streams, ODD_W, rows_for_chunks(21, ODD_W) * ODD_W)


def ties_even():
    n = 12 * CHUNK
    streams = [_tie_stream(seed, n, 1100, 300, 11 * CHUNK) for seed in (4, 5, 6)]
    return frame_of(streams, EVEN_W, rows_for_chunks(12, EVEN_W) * EVEN_W)


# 6 ---- tiny accumulator
def tiny():
    n = 6 * CHUNK
    rng = np.random.default_rng(6)
    streams = []
    for c in range(3):
        s = np.zeros(n, np.uint8)
        for k in range(4):  # 4 chunks x 4 pixels of 1..3: at most 48 / 255 < 0.25
            s[k * CHUNK + rng.choice(CHUNK, 4, replace=False)] = rng.integers(1, 4, 4)
        p = 4 * CHUNK + 3000 + 2000 * c  # then past 0.25 in the middle of chunk 4, behind its head
        s[p : p + 3000] = rng.integers(0, 30 + 100 * c, 3000)
        streams.append(s)
    return frame_of(streams, ODD_W, rows_for_chunks(6, ODD_W) * ODD_W)


# 7 ---- frame tails.  npx = 2 * 16384 + r (r = 0: two whole chunks)
TAILS = {0: (32, 1024), 1: (9, 3641), 15: (1, 32783), 16: (16, 2049), 17: (5, 6557)}


def tail(r):
    H, W = TAILS[r]
    npx = H * W
    assert npx % CHUNK == r and npx // CHUNK == 2
    rng = np.random.default_rng([7, r])
    z = {0: 1, 1: 1, 15: 8, 16: 16, 17: 17}[r]
    red = np.full(npx, 255, np.uint8)  # lands on 16384 at pixel z + 16383, inside the tail chunk (r = 0: the second chunk)
    red[:z] = 0
    green = rng.integers(0, 256, npx, dtype=np.uint8)
    blue = rng.integers(0, 3, npx, dtype=np.uint8) * (rng.random(npx) < 0.001)  # stays below 0.25: every chunk is headed
    blue[-1] = 3
    return frame_of([red, green, blue], W, npx)


# 8 ---- saturation
SAT_SHAPE = (4099, 4096)  # 2^24 + 12288 pixels


def saturation():
    H, W = SAT_SHAPE
    out = np.empty((H * W, 3), np.uint8)
    out[:, 0] = 255
    out[:, 1] = 254
    out[0::2, 2] = 255
    out[1::2, 2] = 254
    out = out.reshape(H, W, 3)
    out.setflags(write=False)
    return out


# 9 ---- the threshold at 64 x 64
T05 = F32(0.05)
TH_START = 3696  # the bright run: 400 pixels behind this one


def _threshold_plane(n128, n_hi):
    s = np.zeros(64 * 64, np.uint8)
    s[:n_hi] = 1
    s[TH_START : TH_START + 400 - n128] = 127
    s[TH_START + 400 - n128 :] = 128
    return s


def threshold_triple():
    """((n128, n_hi) below, at, above): planes whose sequential float32 means are float32(0.05) - 1 ulp, float32(0.05) and
    float32(0.05) + 1 ulp.  Searched, not stated: the sums of the leading ones for every n_hi at once, then 400 vector adds."""
    def search():
        want = [np.nextafter(T05, F32(0)), T05, np.nextafter(T05, F32(1))]
        found = {}
        ones = np.concatenate([[F32(0)], np.add.accumulate(np.full(TH_START, F32(1) / F32(255)), dtype=F32)])
        n_hi = np.arange(1200, 1500)
        for n128 in range(0, 401):
            s = ones[n_hi].copy()
            for i in range(400):
                s = s + (F32(127) / F32(255) if i < 400 - n128 else F32(128) / F32(255))
            mean = (s.astype(np.float64) / 4096.0).astype(F32)
            for k, w in enumerate(want):
                hit = np.flatnonzero(mean == w)
                if hit.size and k not in found:
                    found[k] = (n128, int(n_hi[hit[0]]))
            if len(found) == 3:
                break
        return [found[k] for k in range(3)]

    return _cached("triple", search)


def threshold_frame(which, channel):
    """which: 0 below, 1 at, 2 above; the plane on `channel` (1 green, 2 blue), the other two black."""
    out = np.zeros((64, 64, 3), np.uint8)
    out.reshape(-1, 3)[:, channel] = _threshold_plane(*threshold_triple()[which])
    out.setflags(write=False)
    return out


def equal_planes(which):
    """`gb`: identical G and B planes far above R + 0.05; `gb_plus`: one B pixel one level up; `gr`: identical G and R."""
    rng = np.random.default_rng(9)
    plane = rng.integers(60, 200, (64, 64), dtype=np.uint8)
    out = np.zeros((64, 64, 3), np.uint8)
    out[:, :, 1] = plane
    if which == "gr":
        out[:, :, 0] = plane
        out[:, :, 2] = plane // 2
    else:
        out[:, :, 0] = plane // 4
        out[:, :, 2] = plane
        if which == "gb_plus":
            out[17, 23, 2] += 1
    out.setflags(write=False)
    return out


# 10 ---- the threshold at pipeline size: 264 x 512, a pair of frames one level of one pixel apart on either side of 0.05
PIPE_SHAPE = (264, 512)


def classify(u8):
    from oracle import uwie_oracle as orc

    return orc.classify_cast(orc.normalise_u8(u8))


def threshold_pair(kind):
    """(normal frame, `kind` frame): R noise near 100, the cast channel 12 levels above it with the first k (normal) and
    k + 1 (cast) pixels of a seeded order one level higher still; k found by bisection (the sequential sum is monotone in
    every pixel, so is the decision), then verified by the caller."""
    def make():
        H, W = PIPE_SHAPE
        ch = {"greenish": 1, "bluish": 2}[kind]
        rng = np.random.default_rng([10, ch])
        yy, xx = np.mgrid[0:H, 0:W]
        red = np.clip(100 + 12 * np.sin(xx / 31.0) * np.cos(yy / 19.0) + rng.normal(0, 6, (H, W)), 40, 200).astype(np.uint8)
        base = np.zeros((H, W, 3), np.uint8)
        base[:, :, 0] = red
        base[:, :, ch] = red + 12
        base[:, :, 3 - ch] = red + 6
        order = rng.permutation(H * W)

        def frame(k):
            f = base.copy()
            f.reshape(-1, 3)[order[:k], ch] += 1
            return f

        lo, hi = 0, H * W
        assert classify(frame(lo)) == "normal" and classify(frame(hi)) == kind
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if classify(frame(mid)) == kind:
                hi = mid
            else:
                lo = mid
        a, b = frame(lo), frame(hi)
        a.setflags(write=False)
        b.setflags(write=False)
        return a, b

    return _cached(("pair", kind), make)


# 11 ---- k_chunk_ulps blocks across frames: five frames of 7 chunks each, 35 chunks = 16 + 16 + 3
SEVEN = (114, ODD_W)  # 114 114 pixels: 6 chunks and 15 810 pixels


def seven_chunks(i):
    H, W = SEVEN
    npx = H * W
    assert -(-npx // CHUNK) == 7
    rng = np.random.default_rng([11, i])
    if i == 0:
        px = rng.integers(0, 256, (npx, 3), dtype=np.uint8)
    elif i == 1:
        px = rng.integers(0, 40, (npx, 3), dtype=np.uint8)
    elif i == 2:
        px = np.stack([_tie_stream(20 + c, npx, 1100, 200, 6 * CHUNK) for c in range(3)], axis=1)
    elif i == 3:
        px = rng.integers(200, 256, (npx, 3), dtype=np.uint8)
        px[: 3 * CHUNK + 77] = 0
    else:
        px = (rng.integers(0, 256, (npx, 3)) * (rng.random((npx, 3)) < 0.01)).astype(np.uint8)
    return frame_of(list(px.T), W, npx)


# 12 ---- shapes of the fused chunk pass (k_chunk_hist_quad) that tests/test_gpu_entry_fuse.py lacks
FUSED_SHAPES = [(6, 16384), (1030, 64), (333, 264)]


def fused_frame(i):
    H, W = FUSED_SHAPES[i]
    rng = np.random.default_rng([12, i])
    yy, xx = np.mgrid[0:H, 0:W]
    f = 0.5 + 0.25 * np.sin(xx / (17.0 + 40 * i)) * np.cos(yy / (11.0 - 4 * i))
    gains = [(0.45, 0.85, 0.80), (0.35, 0.6, 1.0), (0.7, 0.72, 0.69)][i]
    img = f[:, :, None] * np.array(gains) + rng.normal(0, 0.02, (H, W, 3))
    out = np.clip(np.floor(255 * img), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- the table
_BUILDERS = [
    ("walk_a", 1, walk_a),
    ("walk_b", 1, walk_b),
    ("drill_positions", 2, drill_positions),
    ("several_binades", 3, several_binades),
    ("landings_128", 4, landings_128),
    ("landings_shifted", 4, landings_shifted),
    ("ties", 5, ties),
    ("ties_even", 5, ties_even),
    ("tiny", 6, tiny),
    *[(f"tail_{r}", 7, (lambda r=r: tail(r))) for r in TAILS],
    ("saturation", 8, saturation),
    *[(f"threshold_{c}_{w}", 9, (lambda w=i, c=ch: threshold_frame(w, c)))
      for ch, c in ((1, "green"), (2, "blue")) for i, w in enumerate(("below", "at", "above"))],
    *[(f"equal_{w}", 9, (lambda w=w: equal_planes(w))) for w in ("gb", "gb_plus", "gr")],
    *[(f"pair_{k}_{w}", 10, (lambda k=k, i=i: threshold_pair(k)[i]))
      for k in ("greenish", "bluish") for i, w in enumerate(("normal", "cast"))],
    *[(f"seven_{i}", 11, (lambda i=i: seven_chunks(i))) for i in range(5)],
    *[(f"fused_{h}x{w}", 12, (lambda i=i: fused_frame(i))) for i, (h, w) in enumerate(FUSED_SHAPES)],
]
NAMES = [name for name, _, _ in _BUILDERS]
GROUP = {name: group for name, group, _ in _BUILDERS}

# what detect_image_type has to say about the threshold cases (asserted against the oracle by tests/test_cast_cases.py)
KINDS = {
    "threshold_green_below": "normal", "threshold_green_at": "normal", "threshold_green_above": "greenish",
    "threshold_blue_below": "normal", "threshold_blue_at": "normal", "threshold_blue_above": "bluish",
    "equal_gb": "normal", "equal_gb_plus": "bluish", "equal_gr": "normal",
    "pair_greenish_normal": "normal", "pair_greenish_cast": "greenish",
    "pair_bluish_normal": "normal", "pair_bluish_cast": "bluish",
}


def case(name) -> Case:
    def make():
        build = {n: b for n, _, b in _BUILDERS}[name]
        u8 = build()
        assert u8.dtype == np.uint8 and u8.ndim == 3 and u8.shape[2] == 3 and not u8.flags.writeable
        return Case(name, GROUP[name], u8)

    return _cached(("case", name), make)


def report(name, channel) -> Report:
    return _cached(("report", name, channel), lambda: events(case(name).u8[:, :, channel]))


def sequential_mean(name):
    """float32 [3]: the analyser's sequential sums divided in float64 and rounded, NumPy's img.mean(axis=(0, 1))."""
    return np.array([report(name, c).mean for c in range(3)], F32)


def general_float_images():
    """name -> float32 (H, W, 3) images that are not u8 / 255, for the general-float route (k_f_mean_seq)."""
    rng = np.random.default_rng(13)
    out = {}
    for H, W in ((5, 7), (61, 83), (128, 128), (300, 400)):
        out[f"uniform_{H}x{W}"] = rng.random((H, W, 3), dtype=F32)
    x = rng.random((97, 131, 3), dtype=F32) * F32(0.3)
    x[:, :, 1] = x[:, :, 0] + F32(0.05)  # green = red + 0.05 pixel by pixel: the decision hangs on the roundings of the two sums
    out["near_threshold_97x131"] = x
    x = rng.random((120, 160, 3), dtype=F32)
    x[rng.random(x.shape) < 0.3] = 0
    tiny_ = rng.random(x.shape) < 0.3
    x[tiny_] = (rng.integers(1, 1 << 23, int(tiny_.sum())).astype(np.uint32)).view(F32)  # subnormals
    out["subnormals_120x160"] = x
    for v in out.values():
        v.setflags(write=False)
    return out
