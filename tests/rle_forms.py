"""Packaging sweep: the run-length kernels of csrc/rle.hip (rle_labels, rle_transitions, rle_compress in its sizing, writing and capped
passes, decode_masks) and the host compressors, held to COCO at every partition boundary.  Everything here is integer and exact: a
comparison is equality, there is no tolerance.

This module holds the case builders, the numpy references and two numpy emulations of the partitioned algorithms; it runs no kernel.
References, none of which shares code with what they judge:
  flips    np.flatnonzero(np.diff(np.concatenate([[0], lab == p])) != 0) on the 1-D label array
  strings  oracle/rle_oracle.py to_string / to_bbox on run lists (the oracle restates cocoapi; its parity with pycocotools is unpinned)
  labels   a numpy look-up table and a transpose
The emulations restate the kernels' partitions (lanes of 16 pixels, steps of 1024, waves of Q pixels; chunks of 256 runs) so that the
CPU half can plant one error at a time and show that the case list notices it.
"""
import numpy as np

from oracle import rle_oracle as R

SENTINEL = 0x7FFFFFFF            # prefill of the positions buffers
FILL = 0xA5                      # prefill of the byte buffers
GAP = 3                          # sentinel words between two masks' position ranges
GUARD = 64                       # sentinel words / bytes after the last range
NONE = 0xFF                      # label of a pixel no kept plane owns
TW = 16                          # waves per workgroup of rle_transitions_kernel


def wave_range(N):
    """Q: the pixels one wave of rle_transitions_kernel owns."""
    return ((N + TW * 1024 - 1) // (TW * 1024)) * 1024


# ------------------------------------------------------------------------------------------------------------------- 1. rle_transitions
TRANSITION_SIZES = (1, 15, 16, 17, 1023, 1024, 1025, 1040, 16383, 16384, 16385, 16400, 32768, 32784, 49168)
OFFSET_BYTE_SIZES = (1040, 16400)            # N % 16 == 0, run from a storage offset of one byte: the scalar path by alignment alone


def flips_ref(lab, p):
    return np.flatnonzero(np.diff(np.concatenate([[0], (np.asarray(lab) == p).astype(np.int8)])) != 0)


def _boundaries(N, period, shift):
    """Plane 0 in alternating runs of `period` pixels, a run boundary at period * k + shift for every k >= 1 (shift 0: also none at 0)."""
    return (((np.arange(N) - shift) // period) % 2 == 1)


def transition_patterns(N):
    """name -> bool [N], the pixels of plane 0."""
    Q = wave_range(N)
    i = np.arange(N)
    rng = np.random.default_rng(N)
    pats = {"none": np.zeros(N, bool), "all": np.ones(N, bool), "first": i == 0, "last": i == N - 1, "even": i % 2 == 0,
            "random .5": rng.random(N) < 0.5, "random .01": rng.random(N) < 0.01}
    for name, period in (("16", 16), ("1024", 1024), ("Q", Q)):
        for shift in (-1, 0, 1):
            pats["%s k %+d" % (name, shift)] = _boundaries(N, period, shift)
    return pats


def transition_case(N):
    """One launch per size: every pattern is a view, once against the other kept label (1) and once against NONE.
    -> (names, lab uint8 [V, N], n_kept int32 [V], nq).  n_kept alternates 2 / 3 of nq = 3: plane 2 is kept and absent, or not kept."""
    names, rows = [], []
    for name, m in transition_patterns(N).items():
        for other in (1, NONE):
            names.append("%s / %s" % (name, "1" if other == 1 else "none"))
            rows.append(np.where(m, 0, other).astype(np.uint8))
    lab = np.stack(rows)
    n_kept = np.array([2 + (v % 2) for v in range(len(rows))], np.int32)
    return names, lab, n_kept, 3


def byte_compare_case():
    """N = 4096 + 16, nq = n_kept = 128: view 0 holds every byte value b at every position j of a 16-byte load (load i = i, i+1, ...,
    i+15 mod 256, so 0xFF sits next to 0x00 and 0x00 next to 0x01), view 1 every value 16 times; the last 16 bytes are the pairs the
    no-borrow claim of rle_eq16 is about (0xFF / 0x7F against p = 127, p ^ 0x80, 0x00 / 0x01)."""
    k = np.arange(4096)
    tail = np.array([0xFF, 0x7F, 0xFF, 0x7F, 0x00, 0x01, 0x00, 0x01, 0x80, 0x00, 0x80, 0x00, 0x7F, 0x80, 0xFE, 0xFF], np.uint8)
    lab = np.stack([np.concatenate([((k // 16 + k % 16) % 256).astype(np.uint8), tail]),
                    np.concatenate([(k // 16).astype(np.uint8), tail[::-1]])])
    return lab, np.array([128, 128], np.int32), 128


def slot_case(N):
    """V = 3, nq = 5, n_kept = 0, 1, nq over one random map of labels 0..4 and NONE."""
    rng = np.random.default_rng(N + 7)
    lab = rng.integers(0, 6, (3, N)).astype(np.uint8)
    lab[lab == 5] = NONE
    return lab, np.array([0, 1, 5], np.int32), 5


def transition_layout(lab, n_kept, nq):
    """Reference counts and the positions buffer both passes are held to: -> (counts int32 [V, nq], offsets int64 [V, nq], expected
    int32 [size]).  Every mask's range holds its reference flips; GAP sentinel words separate consecutive ranges, GUARD follow the last
    (and GAP precede the first), so a write outside a mask's own range changes a word that must still hold the sentinel."""
    V = lab.shape[0]
    counts = np.zeros((V, nq), np.int32)
    offsets = np.zeros((V, nq), np.int64)
    parts, at = [np.full(GAP, SENTINEL, np.int64)], GAP
    for v in range(V):
        for p in range(nq):
            f = flips_ref(lab[v], p) if p < n_kept[v] else np.zeros(0, np.int64)
            counts[v, p], offsets[v, p] = f.size, at
            parts += [f, np.full(GAP, SENTINEL, np.int64)]
            at += f.size + GAP
    parts.append(np.full(GUARD, SENTINEL, np.int64))
    return counts, offsets, np.concatenate(parts).astype(np.int32)


def worst_case_winner(V, H, W):
    """Winner map [V, H, W] (pass bit set) whose column-major neighbours always differ, ids 0 / 1 both kept: plane 0 flips at every
    pixel and plane 1 at every pixel but the first, 2 H W - 1 flips per view - the bound PendingRLE sizes its buffer by is 2 H W."""
    y, x = np.mgrid[0:H, 0:W]
    ids = ((x * H + y) % 2).astype(np.uint8)
    return np.broadcast_to(ids | 0x80, (V, H, W)).copy(), np.tile(np.array([0, 1], np.int32), (V, 1)), np.full(V, 2, np.int32)


# ------------------------------------------------------------------------------------------------------------------------ 2. rle_labels
LABEL_H, LABEL_W, LABEL_NQ = (1, 31, 32, 33, 65), (1, 31, 32, 33), (1, 50, 128)


def labels_case(H, W, nq):
    """V = 3: view 0 keeps nothing, view 1 is a fallback view (flags 2) with a middle n_kept, view 2 a plain view that keeps all nq
    (flags 1: a bit that is not the fallback bit).  Kept ids in random order, 127 among them when nq = 128, -1 in the unused tail; winner
    ids over all of 0..127 (so ids no plane keeps), pass bit random.  -> winner [3, H, W] uint8, kept int32 [3, nq], n_kept, flags."""
    rng = np.random.default_rng(H * 1000 + W * 10 + nq)
    winner = (rng.integers(0, 128, (3, H, W)) | (rng.integers(0, 2, (3, H, W)) << 7)).astype(np.uint8)
    n_kept = np.array([0, (nq + 1) // 2, nq], np.int32)
    kept = np.full((3, nq), -1, np.int32)
    for v in range(3):
        ids = rng.permutation(nq)[:n_kept[v]]
        if nq == 128 and n_kept[v] and 127 not in ids:
            ids[0] = 127
        kept[v, :n_kept[v]] = ids
    winner[:, 0, 0] = (winner[:, 0, 0] & 0x80) | min(nq - 1, 127)       # the highest id a view can keep is present
    return winner, kept, n_kept, np.array([0, 2, 1], np.int32)


def labels_ref(winner, kept, n_kept, flags):
    """uint8 [V, W, H]: ordinal of the kept plane that owns the pixel, NONE otherwise; column-major."""
    V, H, W = winner.shape
    nq = kept.shape[1]
    out = np.empty((V, W, H), np.uint8)
    for v in range(V):
        lut = np.full(128, NONE, np.uint8)
        for t in range(min(int(n_kept[v]), nq)):
            if 0 <= kept[v, t] < 128:
                lut[kept[v, t]] = t
        ok = np.ones((H, W), bool) if flags[v] & 2 else (winner[v] & 0x80) != 0
        out[v] = np.where(ok, lut[winner[v] & 0x7F], NONE).T
    return out


def clamp_case():
    """n_kept[0] = 8 with nq = 6, strictly in bounds (the two entries past view 0's row are view 1's first two, which view 0 keeps
    too, at other ordinals): view 0's labels must be those of n_kept[0] = 6.  -> winner, kept, n_kept (as passed), n_kept (clamped)."""
    rng = np.random.default_rng(6)
    winner = (rng.integers(0, 8, (2, 33, 31)) | 0x80).astype(np.uint8)
    kept = np.array([[0, 1, 2, 3, 4, 5], [1, 3, 0, 2, 6, 7]], np.int32)
    flags = np.zeros(2, np.int32)
    return winner, kept, np.array([8, 6], np.int32), np.array([6, 6], np.int32), flags


# ---------------------------------------------------------------------------------------------------------------------- 3. rle_compress
RUN_COUNTS = (1, 2, 3, 4, 5, 255, 256, 257, 258, 259, 511, 512, 513, 1025)
# stored value -> characters it needs (5 data bits each, the last one's bit 4 is the sign): both sides of every length step
CHARS = {-2**24 - 1: 6, -2**24: 5, -2**19 - 1: 5, -2**19: 4, -2**14 - 1: 4, -2**14: 3, -513: 3, -512: 2, -17: 2, -16: 1, -1: 1, 0: 1, 15: 1,
         16: 2, 511: 2, 512: 3, 2**14 - 1: 3, 2**14: 4, 2**19 - 1: 4, 2**19: 5, 2**24 - 1: 5, 2**24: 6}
MAX_PIXELS = 2**26               # above it a count may need 7 characters; rle.compress sizes its buffer at 6 per run


def chars_needed(x):
    n = 1
    while not -(1 << (5 * n - 1)) <= x < (1 << (5 * n - 1)):
        n += 1
    return n


def _close(runs, H):
    """Lengthen the last run until the runs cover a whole number of columns of height H: -> (runs, H, W)."""
    runs = [int(r) for r in runs]
    runs[-1] += -sum(runs) % H
    return runs, H, sum(runs) // H


def _case(name, runs, H, W):
    assert sum(runs) == H * W <= MAX_PIXELS and all(r > 0 for r in runs[1:]) and runs[0] >= 0, name
    return {"name": name, "runs": runs, "H": H, "W": W}


def _from_mask(name, mask):
    return _case(name, R.run_lengths(mask), *mask.shape)


def extremes_masks():
    """Two masks of 1025 runs whose box extremes come from runs in different waves of chunks other than the first (a run j sits in
    chunk j // 256, wave (j % 256) // 64).  The scan is column-major, so min-x always comes from run 0 / 1 and max-x from the last
    ones-run (here 1023: chunk 3, wave 3); what can move is min-y (run 395: chunk 1, wave 2), max-y (run 601: chunk 2, wave 1) and
    the run that crosses a column (run 901: chunk 3, wave 2), which overrides both, hence the second mask."""
    a = np.zeros((64, 513), bool)
    a[20:41, :512] = True
    a[3:31, 197] = True
    a[25:61, 300] = True
    b = np.zeros((64, 514), bool)
    b[20:41, :513] = True
    b[20:, 450] = True
    b[:41, 451] = True
    return a, b


def compress_cases():
    """Every string / box case, as run lists (runs[0] may be 0: the mask starts with ones; every other run is positive, which is what
    flip positions can express)."""
    cases = []
    for m in RUN_COUNTS:                                     # lengths 1 + 5 j mod 17: run j and run j - 2 always differ (by 10 or -7)
        cases.append(_case("m=%d" % m, *_close([1 + (5 * j) % 17 for j in range(m)], 7)))
    for m in (2, 4, 5, 258, 513):
        cases.append(_case("m=%d first run 0" % m, *_close([0] + [1 + (5 * j) % 17 for j in range(1, m)], 7)))
    for x in CHARS:
        if x > 0:                                            # as a raw count: index 0, 1, 2
            cases.append(_case("raw %d at 0" % x, *_close([x, 3, 5, 4], 64)))
            cases.append(_case("raw %d at 1" % x, *_close([2, x, 5, 4], 64)))
            cases.append(_case("raw %d at 2" % x, *_close([2, 3, x, 4, 6], 64)))
        a, b = (1 - x, 1) if x < 0 else (1, 1 + x)           # as a delta: run j = run j - 2 + x at j = 3 (ones) and j = 4 (zeros)
        cases.append(_case("delta %d at 3" % x, *_close([5, a, 7, b, 9, 11], 64)))
        cases.append(_case("delta %d at 4" % x, *_close([5, 3, a, 2, b, 4, 6], 64)))
    H, W = 5, 7

    def mask(*flat_ranges, shape=(H, W)):
        f = np.zeros(shape[0] * shape[1], bool)
        for lo, hi in flat_ranges:
            f[lo:hi] = True
        return f.reshape(shape, order="F")
    cases.append(_from_mask("pixel (0, 0)", mask((0, 1))))
    cases.append(_from_mask("pixel (H-1, W-1)", mask((H * W - 1, H * W))))
    cases.append(_from_mask("run ends on the last row", mask((3 * H + 2, 4 * H))))
    cases.append(_from_mask("run starts on the first row", mask((3 * H, 3 * H + 3))))
    cases.append(_from_mask("run crosses one column", mask((2 * H + 3, 3 * H + 2))))
    cases.append(_from_mask("run crosses many columns", mask((1 * H + 3, 4 * H + 2))))
    cases.append(_from_mask("H = 1", mask((2, 5), (7, 8), shape=(1, 9))))
    cases.append(_from_mask("W = 1", mask((2, 5), (7, 9), shape=(9, 1))))
    a, b = extremes_masks()
    cases.append(_from_mask("extremes: min-y run 395, max-y run 601", a))
    cases.append(_from_mask("extremes: crossing run 901", b))
    return cases


def batch_masks():
    """Twelve masks of one size for one call; empty masks (no flip position) sit between the others."""
    H, W = 64, 514
    rng = np.random.default_rng(12)
    a, b = extremes_masks()
    z = np.zeros((H, W), bool)
    first, last, blob = z.copy(), z.copy(), z.copy()
    first[0, 0], last[-1, -1] = True, True
    blob[10:50, 100:400] = True
    blob[20:30, 200:220] = False
    masks = [np.pad(a, ((0, 0), (0, 1))), z, b, np.ones((H, W), bool), z, rng.random((H, W)) < 0.01, first, z, last, blob,
             rng.random((H, W)) < 0.015, z]
    return [_from_mask("batch %d" % i, m) for i, m in enumerate(masks)]


def positions_of(runs):
    return np.cumsum(runs)[:-1].astype(np.uint32)


def string_ref(case):
    return R.to_string(case["runs"])


def bbox_ref(case):
    return R.to_bbox({"size": [case["H"], case["W"]], "counts": string_ref(case)}).tolist()


def mask_of(case):
    """bool [H, W] of a case's runs."""
    runs = np.asarray(case["runs"])
    return np.repeat((np.arange(runs.size) & 1).astype(bool), runs).reshape((case["H"], case["W"]), order="F")


def bits_of(case):
    """(words int32 [ceil(H W / 32)], area): bit p & 31 of word p >> 5 is pixel p of the column-major scan."""
    flat = mask_of(case).reshape(-1, order="F")
    packed = np.packbits(flat, bitorder="little")
    packed = np.concatenate([packed, np.zeros(-packed.size % 4, np.uint8)])
    return packed.view(np.uint32).view(np.int32), int(flat.sum())


def positions_layout(cases):
    """The cases' flip positions in one buffer with GAP sentinel words around every mask: -> (positions int32, offsets int64, counts)."""
    parts, offsets, counts, at = [np.full(GAP, SENTINEL, np.int64)], [], [], GAP
    for c in cases:
        pos = positions_of(c["runs"]).astype(np.int64)
        offsets.append(at)
        counts.append(pos.size)
        parts += [pos, np.full(GAP, SENTINEL, np.int64)]
        at += pos.size + GAP
    return np.concatenate(parts).astype(np.int32), np.array(offsets, np.int64), np.array(counts, np.int32)


def capped_caps(lens, k=5):
    """The caps of the capped pass: 0, the end of string k, that minus 1, total - 1, total, total + 5."""
    ends = np.cumsum(lens)
    return [0, int(ends[k]), int(ends[k]) - 1, int(ends[-1]) - 1, int(ends[-1]), int(ends[-1]) + 5]


def capped_expected(strings, cap, size):
    """The byte buffer after the capped pass: the strings that end at or before `cap`, then the prefill."""
    out = np.full(size, FILL, np.uint8)
    at = 0
    for s in strings:
        if at + len(s) <= cap:
            out[at:at + len(s)] = np.frombuffer(s, np.uint8)
        at += len(s)
    return out


# ---------------------------------------------------------------------------------------------------------------------- 4. decode_masks
DECODE_HW = ((1, 1), (3, 5), (4, 4), (1, 17), (63, 65), (64, 64), (17, 241), (16, 257))         # N = 1, 15, 16, 17, 4095, 4096, 4097, 4112


def decode_case(H, W):
    """V = 3, nq = 128: a view that keeps nothing, one that keeps all 128 (random order), a fallback view with 5."""
    rng = np.random.default_rng(H * 300 + W)
    winner = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    n_kept = np.array([0, 128, 5], np.int32)
    kept = np.full((3, 128), -1, np.int32)
    for v in range(3):
        kept[v, :n_kept[v]] = rng.permutation(128)[:n_kept[v]]
    return winner, kept, n_kept, np.array([0, 0, 2], np.int32)


# ------------------------------------------------------------------------------------------------------------------- 5. the emulations
TRANSITION_PLANTS = ("prev lane", "prev step", "prev wave", "wave base", "step base", "tail mask")
COMPRESS_PLANTS = ("j > 1", "x != 0", "delta j-1", "chunk base", "full flag", "even runs", "- (j % 2)")


def _exclusive_within(values, group):
    """Exclusive running sum of `values` that restarts wherever `group` (non-decreasing) changes."""
    c = np.cumsum(values) - values
    start = np.concatenate([[True], group[1:] != group[:-1]])
    return c - np.maximum.accumulate(np.where(start, c, 0))


def emulate_transitions(lab, p, plant=None):
    """rle_transitions_kernel for one (view, plane) in numpy: a lane takes 16 pixels and the pixel before them, a wave sweeps its Q
    pixels 1024 at a time, a flip is written at wave base + step base + the lane's exclusive count in the step + its rank in the lane.
    -> (count, int64 [count + 1]: what the writing pass leaves in a sentinel-filled range; the last word shows a write past it)."""
    lab = np.asarray(lab)
    N, Q = lab.size, wave_range(lab.size)
    nl = (N + 15) // 16
    m = np.zeros(nl * 16, bool)
    m[:N] = lab == p
    m = m.reshape(nl, 16)
    k = np.arange(nl) * 16
    prev = np.concatenate([[False], m[:-1, 15]])
    if plant == "prev lane":
        prev[:] = False
    elif plant == "prev step":
        prev[k % 1024 == 0] = False
    elif plant == "prev wave":
        prev[k % Q == 0] = False
    tr = m ^ np.concatenate([prev[:, None], m[:, :15]], 1)
    if plant != "tail mask":
        tr &= (k[:, None] + np.arange(16)) < N
    cnt = tr.sum(1)
    wave, step = k // Q, k // 1024                                      # Q is a multiple of 1024: a step never straddles two waves
    wave_tot = np.bincount(wave, cnt, TW).astype(np.int64)
    wbase = (np.cumsum(wave_tot) - wave_tot)[wave]
    step_tot = np.bincount(step, cnt).astype(np.int64)
    sbase = _exclusive_within(step_tot, np.arange(step_tot.size) * 1024 // Q)[step]
    lbase = _exclusive_within(cnt, step)
    if plant == "wave base":
        wbase[:] = 0
    elif plant == "step base":
        sbase[:] = 0
    lane_of, j = np.nonzero(tr)                                         # row-major: ascending positions, as the lanes write them
    rank = np.arange(lane_of.size) - (np.cumsum(cnt) - cnt)[lane_of]
    total = int(cnt.sum())
    out = np.full(total + 2, SENTINEL, np.int64)
    out[(wbase + sbase + lbase)[lane_of] + rank] = k[lane_of] + j
    return total, out[:total + 1]


def _chars(x, plant):
    out = []
    more = True
    while more and len(out) < 8:                                        # ("x != 0" never ends on a negative x: eight is the kernel's buffer)
        ch = x & 0x1F
        x >>= 5
        more = (x != (0 if plant == "x != 0" else -1)) if ch & 0x10 else x != 0
        out.append(ch + 48 + (32 if more else 0))
    return out


def emulate_compress(positions, H, W, plant=None):
    """rle_compress_kernel for one mask in numpy / Python: 256 runs per chunk, thread t of a chunk takes run j = j0 + t and reads the
    edges j .. j - 3 (which reach into the previous chunk), the characters land at chunk base + the exclusive scan of the chunk's
    lengths, every thread keeps its own box over the chunks and the workgroup reduces them.  -> (bytes, [x, y, w, h])."""
    pos = [int(q) for q in positions]
    n_pos, N = len(pos), H * W
    m = n_pos + 1
    me = (m // 2) * 2
    edge = lambda j: 0 if j < 0 else (N if j >= n_pos else pos[j])
    xs, ys, xe, ye, full = [W] * 256, [H] * 256, [-1] * 256, [-1] * 256, [0] * 256
    out, base = {}, 0
    for j0 in range(0, m, 256):
        lens, chars = [0] * 256, [None] * 256
        for t in range(256):
            j = j0 + t
            if j >= m:
                continue
            x = edge(j) - edge(j - 1)
            if j > (1 if plant == "j > 1" else 2):
                x -= (edge(j - 1) - edge(j - 2)) if plant == "delta j-1" else (edge(j - 2) - edge(j - 3))
            chars[t] = _chars(x, plant)
            lens[t] = len(chars[t])
            if j < me and not (plant == "even runs" and j % 2):
                e = edge(j) - (0 if plant == "- (j % 2)" else j % 2)
                y = e % H
                xx = (e - y) // H
                if j % 2 == 1:
                    ep = edge(j - 1)
                    if (ep - ep % H) // H < xx and plant != "full flag":
                        full[t] = 1
                xs[t], xe[t], ys[t], ye[t] = min(xs[t], xx), max(xe[t], xx), min(ys[t], y), max(ye[t], y)
        at = base
        for t in range(256):
            for e, ch in enumerate(chars[t] or ()):
                out[at + e] = ch
            at += lens[t]
        base = at if plant != "chunk base" else sum(lens)
    s = bytes(out.get(i, FILL) for i in range(base))
    if me == 0:
        return s, [0.0, 0.0, 0.0, 0.0]
    x0, y0, x1, y1 = min(xs), min(ys), max(xe), max(ye)
    if any(full):
        y0, y1 = 0, H - 1
    return s, [float(x0), float(y0), float(x1 - x0 + 1), float(y1 - y0 + 1)]
