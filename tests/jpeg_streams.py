"""Baseline-JPEG streams no encoder writes, as data: a writer that turns CHOSEN quantised coefficients, quantisation tables and Huffman
specs into a file (ITU T.81 Annex B / F.1.2), and the case tables of tests/test_jpeg_streams_cpu.py and tests/test_jpeg_streams_gpu.py.
The writer knows the coefficients it encoded, so the entropy stage of csrc/jpeg.hip (both Huffman decoders, the DC scan) is held to
something that is not a decoder at all; the pixels of a stream are oracle.jpeg_oracle.reconstruct(parse(data), those coefficients).

Every case generator ASSERTS its own preconditions (the branch it is named after is reached: a code length, a byte phase of a stuffed
FF, a lane count, a bit position against the lane boundary), so that a later edit of the inputs cannot quietly leave the contract:
  * DC differences stay within category 11, AC coefficients within size 10 (the writer refuses anything else);
  * a stream is as long as its case needs (thresholds from nopesac_amd/jpeg.py and include/nopesac_hip.h, never literals);
  * the oracle's sample BEFORE the range limit stays in [-512, 511] in every stream that is compared with Pillow: beyond it
    jidctint.c's range-limit table (the oracle, jpeg_idct_kernel) WRAPS modulo 1024 where libjpeg-turbo's SIMD inverse DCT saturates.
    No conforming encoder writes such blocks; the one family inside that region (`idct_wrap`) is compared with the oracle only.
Imports without a GPU and without Pillow."""
from __future__ import annotations

import functools

import numpy as np

from nopesac_amd import jpeg as P
from oracle import jpeg_oracle as J

ZIGZAG = np.asarray(J.ZIGZAG, np.int64)              # zigzag position k -> natural (row-major) index
SUB_BITS = P.SUB_WORDS * 32                          # one lane of the self-synchronising decoder
SUB_BYTES = SUB_BITS // 8
MIN_PAR = P.PARALLEL_MIN_BYTES                       # shorter restart-free streams stay on the one-wave-per-interval kernel
PASSES = P.SYNC_PASSES
GRAY, S444, S422, S420 = "gray", (1, 1), (2, 1), (2, 2)
EOB, ZRL = 0x00, 0xF0


# ---------------------------------------------------------------------------------------------------------------- Huffman specs
def spec(pairs) -> bytes:
    """[(symbol, code length)] -> BITS[16] + HUFFVAL of a DHT segment (symbols of one length keep their order)."""
    bits = [0] * 16
    vals = []
    for ln in range(1, 17):
        for s, l in pairs:
            if l == ln:
                bits[ln - 1] += 1
                vals.append(s)
    assert len(vals) == len(pairs) == len({s for s, _ in pairs}) and len(vals) <= 256
    out = bytes(bits) + bytes(vals)
    codes(out)
    return out


@functools.lru_cache(maxsize=None)
def codes(sp: bytes) -> dict:
    """symbol -> (code, length): T.81 Annex C canonical codes; the all-ones code of any length stays free (T.81 K.2)."""
    out, code, k = {}, 0, 16
    for ln in range(1, 17):
        for _ in range(sp[ln - 1]):
            assert code < (1 << ln) - 1, "code space exhausted / all-ones code at length %d" % ln
            out[sp[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def _full_ac(order):
    lens = [2, 2, 3, 4, 5, 6] + [7] * 8 + [8] * 16
    return spec([(s, lens[i] if i < len(lens) else 10) for i, s in enumerate(order)])


_COMMON = [EOB, 0x01, 0x02, 0x11, 0x03, 0x21]
_ALL_AC = _COMMON + [(r << 4) | s for s in range(1, 11) for r in range(16) if (r << 4) | s not in _COMMON] + [ZRL]      # the 162 of baseline
# the DC tables of T.81 Annex K.3 (cat 0 at 2 bits ...; the chroma one runs to 11 bits)
DCK0 = spec([(0, 2), (1, 3), (2, 3), (3, 3), (4, 3), (5, 3), (6, 4), (7, 5), (8, 6), (9, 7), (10, 8), (11, 9)])
DCK1 = spec([(0, 2), (1, 2), (2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (7, 7), (8, 8), (9, 9), (10, 10), (11, 11)])
# two full AC tables with different symbol orders (a decoder that takes the other table's id reads garbage): 30 symbols within the 9-bit
# look-ahead, 132 at 10 bits
AC0 = _full_ac(_ALL_AC)
AC1 = _full_ac([EOB] + [_ALL_AC[1 + (37 * i) % 161] for i in range(161)])
# one DC code per length 1 .. 12 (category c: c ones and a zero); categories 9, 10, 11 sit behind the look-ahead
DCL = spec([(c, c + 1) for c in range(12)])
# one AC code per length 1 .. 16; EOB, runs 2 / 3 / 14, ZRL, size 2 and size 10 sit behind the look-ahead, (0, 10) on the 16-bit code
# 0xFFFE: with its ten value bits the 26-bit symbol of the lane-boundary sweep, and 25 ones in a row when the value is +1023
ACL = spec([(0x01, 1), (0x11, 2), (0x03, 3), (0x04, 4), (0x05, 5), (0x06, 6), (0x07, 7), (0x08, 8), (0x09, 9), (EOB, 10), (0x21, 11),
            (0x31, 12), (ZRL, 13), (0x02, 14), (0xE1, 15), (0x0A, 16)])
ACL_SLOW = (EOB, 0x21, 0x31, ZRL, 0x02, 0xE1, 0x0A)
# seven short codes, the other 155 symbols at 16 bits
_SHORT16 = [EOB, 0x01, 0x02, 0x11, 0x03, 0x21, ZRL]
AC16 = spec([(s, i + 1) for i, s in enumerate(_SHORT16)] + [(s, 16) for s in _ALL_AC if s not in _SHORT16])
# one-symbol tables
DC_ONE, AC_EOB_ONLY, AC_ONE = spec([(0, 1)]), spec([(EOB, 1)]), spec([(0x01, 1)])

Q1 = np.ones(64, np.int64)


# ---------------------------------------------------------------------------------------------------------------- the writer
class Stream:
    """One written file.  coef: per component int16 [bh][bw][64], ZIGZAG order, DC resolved, MCU padding included (the layout of the
    device coefficient buffer).  seg_bytes: unstuffed length of every restart interval.  trace (interval 0 only, on request): per
    symbol (first bit, code + value bits, symbol or -1 - category for DC), and the bit every block ends on."""
    __slots__ = ("name", "data", "coef", "qt", "seg_bytes", "scan", "trace", "block_end", "wrap", "W", "H", "sampling", "_px")

    def natural(self):
        out = []
        for c in self.coef:
            n = np.zeros(c.shape, np.int32)
            n[..., ZIGZAG] = c
            out.append(n)
        return out

    def pixels(self):
        """what libjpeg makes of these coefficients (RGB uint8 [H][W][3]); computed once, read-only"""
        if self._px is None:
            fr = J.parse(self.data)
            J.geometry(fr)
            self._px = J.reconstruct(fr, self.natural())
            self._px.setflags(write=False)
        return self._px


def grid(W, H, sampling):
    """-> [(bh, bw)] per component, MCU padding included"""
    if sampling == GRAY:
        return [(-(-H // 8), -(-W // 8))]
    hs, vs = sampling
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    return [(my * vs, mx * hs), (my, mx), (my, mx)]


def zeros(W, H, sampling):
    return [np.zeros((bh, bw, 64), np.int64) for bh, bw in grid(W, H, sampling)]


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def write(name, coef, W, H, sampling=GRAY, qt=(Q1, Q1), tq=(0, 1, 1), dc=(DCK0, DCK1), ac=(AC0, AC1), td=(0, 1, 1), ta=(0, 1, 1), dri=0,
          fill=0, trace=False, wrap=False) -> Stream:
    """coef: per component [bh][bw][64] in zigzag order with the DC value itself (grid()); qt: quantisation tables in zigzag order
    (written with Pq = 1 and under SOF1 when an entry exceeds 255); dc / ac: up to two Huffman specs each; tq / td / ta: the table ids of
    every component; dri: restart interval in MCUs; fill: FF fill bytes in front of every RSTn and of EOI."""
    shapes = grid(W, H, sampling)
    nc = len(shapes)
    assert len(coef) == nc and all(c.shape == (bh, bw, 64) for c, (bh, bw) in zip(coef, shapes)), "coefficient layout"
    hs, vs = (1, 1) if sampling == GRAY else sampling
    mcuy, mcux = shapes[0][0] // vs, shapes[0][1] // hs
    dcc, acc_ = [codes(t) for t in dc], [codes(t) for t in ac]
    tq, td, ta = tq[:nc], td[:nc], ta[:nc]
    st = Stream()
    st.name, st.W, st.H, st.sampling, st.wrap, st._px = name, W, H, sampling, wrap, None
    st.coef = [np.asarray(c).astype(np.int16) for c in coef]
    st.qt = [np.asarray(qt[t], np.int64) for t in tq]
    st.trace, st.block_end = ([], []) if trace else (None, None)
    cl = [c.tolist() for c in coef]
    n_mcu = mcux * mcuy
    per = dri if dri else n_mcu
    parts, st.seg_bytes = [], []
    for first in range(0, n_mcu, per):
        tr = trace and first == 0
        pred = [0] * nc
        bits = []                                          # (value, length) of the interval, packed below
        pos = 0
        for m in range(first, min(first + per, n_mcu)):
            my, mx = divmod(m, mcux)
            for ci in range(nc):
                ch, cv = (hs, vs) if ci == 0 else (1, 1)
                D, A = dcc[td[ci]], acc_[ta[ci]]
                for v in range(cv):
                    for h in range(ch):
                        blk = cl[ci][my * cv + v][mx * ch + h]
                        d = blk[0] - pred[ci]
                        pred[ci] = blk[0]
                        s = abs(d).bit_length()
                        assert s <= 11, "DC difference %d beyond category 11" % d
                        assert s in D, "DC category %d not in the table" % s
                        c, l = D[s]
                        bits.append(((c << s) | (d if d >= 0 else d + (1 << s) - 1), l + s))
                        if tr:
                            st.trace.append((pos, l + s, -1 - s))
                        pos += l + s
                        run = 0
                        for k in range(1, 64):
                            x = blk[k]
                            if x == 0:
                                run += 1
                                continue
                            while run > 15:
                                assert ZRL in A, "ZRL not in the table"
                                bits.append(A[ZRL])
                                if tr:
                                    st.trace.append((pos, A[ZRL][1], ZRL))
                                pos += A[ZRL][1]
                                run -= 16
                            s = abs(x).bit_length()
                            assert s <= 10, "AC coefficient %d beyond size 10" % x
                            assert (run << 4 | s) in A, "AC symbol %02X not in the table" % (run << 4 | s)
                            c, l = A[run << 4 | s]
                            bits.append(((c << s) | (x if x >= 0 else x + (1 << s) - 1), l + s))
                            if tr:
                                st.trace.append((pos, l + s, run << 4 | s))
                            pos += l + s
                            run = 0
                        if run:
                            assert EOB in A, "EOB not in the table"
                            bits.append(A[EOB])
                            if tr:
                                st.trace.append((pos, A[EOB][1], EOB))
                            pos += A[EOB][1]
                        if tr:
                            st.block_end.append(pos)
        big, n = 0, 0
        out = bytearray()
        for val, ln in bits:                               # pack in chunks: one big-int shift per symbol on a bounded accumulator
            big = (big << ln) | val
            n += ln
            if n >= 4096:
                keep = n & 7
                out += (big >> keep).to_bytes((n - keep) // 8, "big")
                big &= (1 << keep) - 1
                n = keep
        pad = (-n) % 8
        big = (big << pad) | ((1 << pad) - 1)              # the last byte is completed with one bits (T.81 F.1.2.3)
        out += big.to_bytes((n + pad) // 8, "big")
        assert len(out) == -(-pos // 8)
        parts.append(bytes(out))
        st.seg_bytes.append(len(out))
    scan = bytearray()
    for i, q in enumerate(parts):
        scan += q.replace(b"\xff", b"\xff\x00")
        if i + 1 < len(parts):
            scan += b"\xff" * fill + bytes([0xFF, 0xD0 + (i & 7)])
    st.scan = bytes(scan)
    f = bytearray(b"\xff\xd8")
    f += _seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    wide = False
    for t in sorted(set(tq)):
        q = np.asarray(qt[t], np.int64)
        assert q.shape == (64,) and q.min() >= 1 and q.max() <= 65535
        if q.max() > 255:
            wide = True
            f += _seg(0xDB, bytes([0x10 | t]) + q.astype(">u2").tobytes())
        else:
            f += _seg(0xDB, bytes([t]) + q.astype(np.uint8).tobytes())
    sof = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([nc])
    for ci in range(nc):
        ch, cv = (hs, vs) if ci == 0 else (1, 1)
        sof += bytes([ci + 1, (ch << 4) | cv, tq[ci]])
    f += _seg(0xC1 if wide else 0xC0, sof)
    for t in sorted(set(td)):
        f += _seg(0xC4, bytes([t]) + dc[t])
    for t in sorted(set(ta)):
        f += _seg(0xC4, bytes([0x10 | t]) + ac[t])
    if dri:
        f += _seg(0xDD, dri.to_bytes(2, "big"))
    sos = bytes([nc])
    for ci in range(nc):
        sos += bytes([ci + 1, (td[ci] << 4) | ta[ci]])
    f += _seg(0xDA, sos + bytes([0, 63, 0]))
    f += st.scan + b"\xff" * fill + b"\xff\xd9"
    st.data = bytes(f)
    return st


# ---------------------------------------------------------------------------------------------------------------- preconditions
def prelimit(coef, q):
    """jidctint.c's sample before the range limit (what `& RANGE_MASK` sees, 0 = mid grey): coef [..., 64] and q [64] in zigzag order"""
    x = np.zeros(coef.shape, np.int64)
    x[..., ZIGZAG] = np.asarray(coef, np.int64) * np.asarray(q, np.int64)
    x = x.reshape(x.shape[:-1] + (8, 8))
    ws = np.swapaxes(J._idct_1d(np.swapaxes(x, -1, -2), 0, 11), -1, -2)
    return J._idct_1d(ws, 0, 18)


def prelimit_range(st: Stream):
    ys = [prelimit(c, q) for c, q in zip(st.coef, st.qt)]
    return min(int(y.min()) for y in ys), max(int(y.max()) for y in ys)


def in_range(st: Stream) -> Stream:
    lo, hi = prelimit_range(st)
    assert -512 <= lo and hi <= 511, "%s: pre-limit samples %d .. %d leave [-512, 511]" % (st.name, lo, hi)
    return st


def stuffing_profile(scan: bytes):
    """How the three host readers meet the stuffed bytes of a scan: the word phases (unstuffed byte index modulo 4) FF bytes land on,
    the pending byte counts with which a run of plain bytes starts behind an FF (nopesac_jpeg_prepare_scan's bulk copy), the longest
    run of stuffed FFs."""
    phases, pending, longest, run, n, i = set(), set(), 0, 0, 0, 0
    while i < len(scan):
        if scan[i] == 0xFF and i + 1 < len(scan) and scan[i + 1] == 0:
            phases.add(n % 4)
            n += 1
            run += 1
            longest = max(longest, run)
            i += 2
            if i < len(scan) and scan[i] != 0xFF:
                pending.add(n % 4)
        elif scan[i] == 0xFF:
            break                                          # a marker: the profile is of the first interval
        else:
            run = 0
            n += 1
            i += 1
    return phases, pending, longest


def n_lanes(st: Stream) -> int:
    """lanes of the self-synchronising decoder (0: the stream stays on the one-wave-per-interval kernel)"""
    if len(st.seg_bytes) != 1 or st.seg_bytes[0] < MIN_PAR:
        return 0
    return -(-st.seg_bytes[0] * 8 // SUB_BITS)


# ---------------------------------------------------------------------------------------------------------------- block makers
def _rng(seed):
    return np.random.default_rng(seed)


def random_blocks(rng, shape, n_ac=8, amp=3, dc_step=40, dc_lim=200):
    """[..., 64] zigzag blocks: a DC random walk, up to n_ac coefficients of magnitude <= amp anywhere"""
    n = int(np.prod(shape))
    out = np.zeros((n, 64), np.int64)
    dcv = np.clip(np.cumsum(rng.integers(-dc_step, dc_step + 1, n)), -dc_lim, dc_lim)
    out[:, 0] = dcv
    rank = np.argsort(np.argsort(rng.random((n, 63)), 1), 1)                   # a random order of the 63 positions per block
    vals = rng.integers(1, amp + 1, (n, 63)) * rng.choice([-1, 1], (n, 63))
    out[:, 1:] = np.where(rank < rng.integers(0, n_ac + 1, (n, 1)), vals, 0)
    return out.reshape(tuple(shape) + (64,))


def fitted_gray(name, seed, total_bits, bw=16, **kw):
    """A grey stream of EXACTLY total_bits bits (DCK0 / AC0): random blocks, then a tail of 16 .. 31 blocks whose (0, 1) and (0, 2)
    symbols (3 and 5 bits with their values) make up the rest."""
    rng = _rng(seed)
    D, A = codes(DCK0), codes(AC0)
    assert D[0][1] == 2 and A[EOB][1] == 2 and A[0x01][1] == 2 and A[0x02][1] == 3
    blocks, used, pred = [], 0, 0
    while True:
        T = (-len(blocks)) % bw + bw
        rest = total_bits - used
        assert rest >= 4 * T + 8, "overshot: %d bits left for a tail of %d blocks" % (rest, T)
        if rest <= T * (4 + 3 * 50):
            break
        if len(blocks) % 256 == 0:
            pool = random_blocks(rng, (256,))
        b = pool[len(blocks) % 256]
        b[0] = int(np.clip(pred + rng.integers(-40, 41), -200, 200))
        # bits of this block
        d = int(b[0]) - pred
        s = abs(d).bit_length()
        n = D[s][1] + s
        run = 0
        for k in range(1, 64):
            x = int(b[k])
            if x == 0:
                run += 1
                continue
            while run > 15:
                n += A[ZRL][1]
                run -= 16
            s = abs(x).bit_length()
            n += A[run << 4 | s][1] + s
            run = 0
        if run:
            n += A[EOB][1]
        pred = int(b[0])
        used += n
        blocks.append(b)
    extra = total_bits - used - 4 * T                      # = 3 a + 5 b
    nb5 = (2 * extra) % 3
    na3 = (extra - 5 * nb5) // 3
    assert na3 >= 0 and 3 * na3 + 5 * nb5 == extra and na3 + nb5 <= 60 * T
    syms = [2] * nb5 + [1] * na3
    for t in range(T):
        b = np.zeros(64, np.int64)
        b[0] = pred
        take = syms[t * 60:(t + 1) * 60]
        for k, mag in enumerate(take):
            b[1 + k] = (mag + int(rng.integers(0, mag))) * int(rng.choice([-1, 1]))       # magnitude 1, or 2 .. 3
        blocks.append(b)
    bh = len(blocks) // bw
    coef = [np.stack(blocks).reshape(bh, bw, 64)]
    st = write(name, coef, 8 * bw - 3, 8 * bh - 5, GRAY, dc=(DCK0,), ac=(AC0,), td=(0,), ta=(0,), tq=(0,), **kw)
    assert st.seg_bytes == [-(-total_bits // 8)], (st.seg_bytes, total_bits)
    return in_range(st)


# ---------------------------------------------------------------------------------------------------------------- entropy families
def _used_symbols(st):
    return {s for _, _, s in st.trace}


@functools.lru_cache(maxsize=None)
def code_lengths():
    """DCL / ACL: one code per length; every symbol of these streams sits behind the 9-bit look-ahead (DC categories 9 .. 11 at 10 ..
    12 bits, AC symbols at 10 .. 16 bits); AC16: 155 symbols at 16 bits."""
    out = []
    # grey, 64 blocks: DC values whose differences have categories 9, 10, 11; AC: runs 2, 3, 14, ZRL, sizes 2 and 10, EOB
    dcv = [300, -400, 900, 500, -250, -1000, 1000, 620]
    pats = [{3: 1}, {4: -1}, {15: 1}, {19: -1, 20: 2}, {1: 1023}, {1: 2, 5: -1}, {1: -600}, {3: -1, 7: 1, 22: -1, 41: 1}]
    c = zeros(64, 64, GRAY)
    for i in range(64):
        b = c[0][i // 8, i % 8]
        b[0] = dcv[i % 8] + (i // 8)
        for k, v in pats[(i + i // 8) % 8].items():
            b[k] = v
    st = in_range(write("lengths_slow_path", c, 64, 64, GRAY, dc=(DCL,), ac=(ACL,), td=(0,), ta=(0,), trace=True))
    used = _used_symbols(st)
    assert {s for s in used if s < 0} == {-10, -11, -12}, used
    assert {s for s in used if s >= 0} == set(ACL_SLOW), used
    assert all(codes(ACL)[s][1] > P.LOOK_BITS for s in ACL_SLOW) and codes(ACL)[0x0A] == (0xFFFE, 16)
    out.append(st)
    # every code of DCL and ACL at least once (lengths 1 .. 12 and 1 .. 16)
    c = zeros(64, 32, GRAY)
    dc_all = np.cumsum([0, 1, -3, 7, -15, 31, -63, 127, -255, 511, -1023, 1365, -1300, 600] + [0] * 18).tolist()
    acs = [{1: 1}, {2: -1}, {1: 5}, {1: -9}, {1: 17}, {1: -33}, {1: 65}, {1: -129}, {1: 257}, {}, {3: 1}, {4: -1}, {17: 1}, {1: 2}, {15: -1},
           {1: 513}]
    for i in range(32):
        b = c[0][i // 8, i % 8]
        b[0] = dc_all[i]
        for k, v in acs[i % 16].items():
            b[k] = v
    st = in_range(write("lengths_every_code", c, 64, 32, GRAY, dc=(DCL,), ac=(ACL,), td=(0,), ta=(0,), trace=True))
    used = _used_symbols(st)
    assert {-1 - s for s in used if s < 0} == set(range(12)) and {s for s in used if s >= 0} == set(codes(ACL)), used
    out.append(st)
    # AC16: each of the 155 sixteen-bit symbols once, one per block (a coefficient of its size behind its run)
    long16 = [s for s, (_, l) in codes(AC16).items() if l == 16]
    assert len(long16) == 155
    c = zeros(8 * 16, 8 * 10, GRAY)
    for i, s in enumerate(long16):
        b = c[0][i // 16, i % 16]
        r, sz = s >> 4, s & 15
        b[0] = (i % 7) * 30 - 90
        b[20 + r] = (1 << sz) - 1 if i % 2 else -(1 << (sz - 1))
        b[19] = 1
    st = in_range(write("lengths_155_at_16_bits", c, 128, 80, GRAY, dc=(DCK0,), ac=(AC16,), td=(0,), ta=(0,), trace=True))
    assert set(long16) <= _used_symbols(st)
    out.append(st)
    return out


@functools.lru_cache(maxsize=None)
def one_symbol_tables():
    """tables that hold ONE code: DC category 0 only; AC: EOB only (a flat mid-grey image, an all-zero stream) or (0, 1) only (every
    block fills index 63 with +-1 and carries no EOB)"""
    out = [write("one_symbol_eob", zeros(40, 24, GRAY), 40, 24, GRAY, dc=(DC_ONE,), ac=(AC_EOB_ONLY,), td=(0,), ta=(0,))]
    assert out[0].scan == b"\0" * 3 + b"\x03"               # 15 blocks of two zero bits, two padding ones
    rng = _rng(3)
    c = zeros(24, 24, S420)
    for a in c:
        a[..., 1:] = rng.choice([-1, 1], a[..., 1:].shape)
    out.append(in_range(write("one_symbol_full_blocks_420", c, 24, 24, S420, dc=(DC_ONE,), ac=(AC_ONE,), td=(0, 0, 0), ta=(0, 0, 0))))
    return out


@functools.lru_cache(maxsize=None)
def table_ids():
    """the same coefficients under permuted table ids: luma on DC1 / AC1 and chroma on DC0 / AC0; Cb and Cr on different tables; all
    three components on one pair; per sampling mode"""
    out = []
    for si, samp in enumerate((S444, S422, S420)):
        rng = _rng(40 + si)
        W, H = 37, 27
        c = [random_blocks(rng, s) for s in grid(W, H, samp)]
        for nm, td, ta in (("luma1_chroma0", (1, 0, 0), (1, 0, 0)), ("cb0_cr1", (1, 0, 1), (0, 0, 1)), ("cb1_cr0", (0, 1, 0), (1, 1, 0)),
                           ("all_on_0", (0, 0, 0), (0, 0, 0)), ("all_on_1", (1, 1, 1), (1, 1, 1)), ("dc_ac_crossed", (0, 1, 1), (1, 0, 0))):
            out.append(in_range(write("ids_%s_%dx%d" % (nm, samp[0], samp[1]), c, W, H, samp, td=td, ta=ta)))
    return out


@functools.lru_cache(maxsize=None)
def categories():
    """both ends of every category: DC differences of categories 0 .. 11 and AC coefficients of sizes 1 .. 10 with the values
    -(2^s - 1), -2^(s-1), 2^(s-1), 2^s - 1, through each of the table pairs"""
    ends = lambda s: [-(1 << s) + 1, -(1 << (s - 1)), 1 << (s - 1), (1 << s) - 1]
    diffs = [0]
    for s in range(1, 12):
        diffs += ends(s)
    # order the differences so that the running sum stays within [-1024, 1023]
    seq, pred, left = [], 0, sorted(diffs, key=abs, reverse=True)
    while left:
        d = next(d for d in left if -1024 <= pred + d <= 1023)
        left.remove(d)
        pred += d
        seq.append(pred)
    acv = [v for s in range(1, 11) for v in ends(s)]
    out = []
    for nm, D, A in (("annex_k", DCK0, AC0), ("per_length", DCL, ACL), ("sixteen_bit", DCK1, AC16)):
        c = zeros(8 * 9, 8 * 5, GRAY)
        for i in range(45):
            b = c[0][i // 9, i % 9]
            b[0] = seq[i]
            if i < 40:
                b[1] = acv[i]                              # (run 0: the per-length table has no other run for sizes above 1)
        assert c[0][..., 0].min() == -1024 or c[0][..., 0].max() == 1023
        st = in_range(write("categories_" + nm, c, 72, 40, GRAY, dc=(D,), ac=(A,), td=(0,), ta=(0,), trace=True))
        used = _used_symbols(st)
        assert {-1 - s for s in used if s < 0} == set(range(12)) and {s & 15 for s in used if s > 0 and s != ZRL} == set(range(1, 11))
        out.append(st)
    return out


@functools.lru_cache(maxsize=None)
def runs_and_block_ends():
    """ZRL chains of 1, 2 and 3 in front of a coefficient at index 63; a block that fills index 63 (no EOB); blocks with DC only; run 15
    behind a ZRL landing exactly on 63; in grey and in 4:2:0 (chroma through the other tables)"""
    pats = [{63: 1}, {20: 2, 63: -1}, {36: -3, 63: 2}, {63: -7, 31: 1}, {}, {k: (1 if k % 3 else -2) for k in range(1, 64)}, {16: 1}, {17: -1},
            {31: 5, 63: 1}, {}, {47: 1, 63: -1}, {15: 1, 31: -1, 47: 1, 63: -1}]
    out = []
    for samp, W, H in ((GRAY, 32, 24), (S420, 32, 32)):
        c = zeros(W, H, samp)
        i = 0
        for a in c:
            for b in a.reshape(-1, 64):
                b[0] = (i * 37) % 200 - 100
                for k, v in pats[i % len(pats)].items():
                    b[k] = v
                i += 1
        kw = dict(dc=(DCK0,), ac=(AC0,), td=(0,), ta=(0,)) if samp == GRAY else {}
        st = in_range(write("runs_%s" % (samp if samp == GRAY else "420"), c, W, H, samp, trace=True, **kw))
        # the symbols in front of index 63: (14, s) behind three ZRLs, (10, s) behind two, (15, s) behind one
        seq = [s for _, _, s in st.trace if s >= 0]
        text = ",".join("%02X" % s for s in seq)
        assert "F0,F0,F0,E1" in text and "F0,F0,A1" in text and "F0,A2" in text and "F0,F1" in text and "F0,F3" in text, text
        out.append(st)
    return out


@functools.lru_cache(maxsize=None)
def dc_prediction():
    """DC-only images whose prediction runs over more than 256 and more than 1024 blocks of one component with sums swinging between
    -1024 and 1023: jpeg_dc_kernel's 256-block steps and four waves (these streams are long enough for the lanes); in 4:2:0 the scan
    order differs from the block-row order"""
    out = []
    for nm, samp, W, H in (("gray_1120", GRAY, 320, 217), ("420_1156_luma", S420, 265, 270), ("422_300", S422, 150, 75)):
        rng = _rng(len(nm))
        c = zeros(W, H, samp)
        for a in c:
            n = a.shape[0] * a.shape[1]
            v = rng.integers(-1024, 1024, n)
            v[::5] = np.where(np.arange(n)[::5] % 2 == 0, -1024, 1023)
            a[..., 0] = v.reshape(a.shape[:2])
        st = in_range(write("dc_" + nm, c, W, H, samp, dc=(DCL, DCK1), ac=(ACL, AC1)))
        assert n_lanes(st) > 0
        out.append(st)
    assert out[0].coef[0].shape[0] * out[0].coef[0].shape[1] > 1024 and out[1].coef[0].shape[0] * out[1].coef[0].shape[1] > 1024
    assert out[1].coef[1].shape[0] * out[1].coef[1].shape[1] > 256
    return out


@functools.lru_cache(maxsize=None)
def stuffing():
    """FF 00 at every byte phase of a word, as the last bytes of an interval, in runs several bytes long, the bulk copy of
    nopesac_jpeg_prepare_scan entered with 1, 2 and 3 bytes pending, fill FFs in front of RSTn and EOI (DCL / ACL: +1023 behind the
    16-bit code is 25 ones in a row, a DC difference of +2047 eleven)"""
    out = []
    phases, pending = set(), set()
    for i in range(8):
        c = zeros(48, 8, GRAY)
        for j in range(6):
            b = c[0][0, j]
            b[0] = 1023 if j % 2 == 0 else -1024
            b[1] = b[2] = 1023
        c[0][0, 0, 3:3 + i] = 1                            # two bits each: another phase of everything behind them
        c[0][0, 5, 1:63] = np.where(np.arange(62) % 2, 1, -1)
        c[0][0, 5, 63] = 1023                              # the interval ends inside ten one bits: its last byte is FF
        st = in_range(write("stuffing_%d" % i, c, 48, 8, GRAY, dc=(DCL,), ac=(ACL,), td=(0,), ta=(0,), fill=i % 3))
        ph, pe, run = stuffing_profile(st.scan)
        phases |= ph
        pending |= pe
        assert st.scan.endswith(b"\xff\x00") and run >= 2
        out.append(st)
    assert phases == {0, 1, 2, 3} and pending >= {1, 2, 3}, (phases, pending)
    assert any(b"\xff\x00\xff\x00\xff\x00" in s.scan for s in out)
    # with restart markers: every interval ends on a stuffed FF, fill bytes in front of RSTn and EOI
    for fill in (0, 1, 3):
        c = zeros(48, 24, S420)
        for a in c:
            a[..., 0] = 100
            a[..., 1:63] = np.where(np.arange(62) % 2, 1, -1)
            a[..., 63] = 1023
            a[..., 1] = -511
        st = in_range(write("stuffing_rst_fill%d" % fill, c, 48, 24, S420, dc=(DCL, DCL), ac=(ACL, ACL), dri=1, fill=fill))
        assert st.scan.count(b"\xff\x00" + b"\xff" * (fill + 1)) >= 5
        out.append(st)
    return out


@functools.lru_cache(maxsize=None)
def restart_intervals():
    """intervals of 1 MCU, of 1 MCU row, a count that does not divide the MCU count (short last interval), more than 8 intervals (RST7
    wraps to RST0), an interval longer than 512 bytes (both 64-word windows of the bit reader turn over), intervals starting at every
    word offset modulo 4 of the batch's word array"""
    out = []
    for nm, samp, W, H, dri, kw in (("1mcu_gray", GRAY, 40, 24, 1, {}), ("1mcu_420", S420, 50, 40, 1, {}), ("row_422", S422, 70, 30, 5, {}),
                                    ("short_last_444", S444, 45, 28, 7, {}), ("short_last_420", S420, 100, 60, 5, {}),
                                    ("long_gray", GRAY, 256, 40, 70, dict(n_ac=24, amp=40)), ("long_420", S420, 128, 64, 13, dict(n_ac=30, amp=25))):
        rng = _rng(len(out) + 70)
        c = [random_blocks(rng, s, **kw) for s in grid(W, H, samp)]
        st = in_range(write("rst_" + nm, c, W, H, samp, dri=dri, fill=len(out) % 2))
        n_mcu = (st.coef[-1].shape[0] * st.coef[-1].shape[1])
        assert len(st.seg_bytes) == -(-n_mcu // dri)
        out.append(st)
    by = {s.name: s for s in out}
    assert len(by["rst_1mcu_gray"].seg_bytes) > 8 and len(by["rst_1mcu_420"].seg_bytes) > 8
    assert (12 * 4) % 7 and (7 * 4) % 5                                      # short last intervals
    assert min(by["rst_long_gray"].seg_bytes[:-1]) > 512 and max(by["rst_long_420"].seg_bytes) > 512
    offs, o = set(), 0
    for s in out:                                          # the word layout of jpeg._words: whole words + 4 zero words per interval
        for n in s.seg_bytes:
            offs.add(o % 4)
            o += -(-n // 4) + 4
    assert offs == {0, 1, 2, 3}
    return out


# ---------------------------------------------------------------------------------------------------------------- the lane decoder
@functools.lru_cache(maxsize=None)
def lane_thresholds():
    """streams of exactly PARALLEL_MIN_BYTES - 1 and PARALLEL_MIN_BYTES bytes; an exact multiple of SUB bits and one byte longer (a
    last lane of 8 bits)"""
    out = [fitted_gray("below_threshold", 1, 8 * (MIN_PAR - 1) - 3), fitted_gray("at_threshold", 2, 8 * MIN_PAR - 5),
           fitted_gray("multiple_of_sub", 3, 6 * SUB_BITS), fitted_gray("multiple_of_sub_plus_a_byte", 4, 6 * SUB_BITS + 8)]
    assert [n_lanes(s) for s in out] == [0, MIN_PAR // SUB_BYTES, 6, 7]
    assert out[0].seg_bytes == [MIN_PAR - 1] and out[1].seg_bytes == [MIN_PAR] and out[3].seg_bytes == [6 * SUB_BYTES + 1]
    return out


LANE_COUNTS = (63, 64, 65, 256, 257)


@functools.lru_cache(maxsize=None)
def lane_counts():
    """63, 64, 65, 256 and 257 lanes: padding lanes in the last wave, none, one lane in a second wave; the second step of
    jpeg_sync_scan_kernel's 256-wide loop and its carry"""
    out = [fitted_gray("lanes_%d" % n, 10 + n, n * SUB_BITS - 8 * (n % 5) - 3, bw=32) for n in LANE_COUNTS]
    assert tuple(n_lanes(s) for s in out) == LANE_COUNTS
    return out


@functools.lru_cache(maxsize=None)
def lane_boundary():
    """32 images for ONE batch: a chain of blocks that each hold the 26-bit symbol (16-bit code + 10 value bits), behind a first block
    one bit longer from image to image, so that the symbol straddles bit SUB at every one of its bit positions, starts on it, and a
    block ends exactly on it"""
    out, cuts, ends = [], set(), False
    D, A = codes(DCL), codes(ACL)
    period = D[0][1] + 26 + A[EOB][1]                      # a chain block: DC difference 0, (0, 10) + value, EOB
    assert A[0x0A][1] + 10 == 26
    nblk = -(-(8 * MIN_PAR + 64) // period)                # the sweep needs the lanes: a chain as long as the threshold asks
    bw = 16
    bh = -(-nblk // bw)
    for i in range(32):
        c = zeros(8 * bw, 8 * bh, GRAY)
        flat = c[0].reshape(-1, 64)
        flat[:, 1] = np.where(np.arange(bh * bw) % 2 == 0, 1023, -1023)
        flat[:, 0] = 50
        flat[0, 1:] = 0                                    # the first block is i + 2 bits longer than DC + EOB: (1, 1) is 3 bits, (0, 1) is 2
        odd = (i + 2) % 2
        if odd:
            flat[0, 2] = -1
        flat[0, 1 + 2 * odd:1 + 2 * odd + (i + 2 - 3 * odd) // 2] = 1
        st = in_range(write("boundary_%02d" % i, c, 8 * bw, 8 * bh, GRAY, dc=(DCL,), ac=(ACL,), td=(0,), ta=(0,), trace=True))
        assert st.block_end[0] == out[0].block_end[0] + i if out else True
        assert n_lanes(st) >= MIN_PAR // SUB_BYTES
        for p, n, s in st.trace:                           # against every lane boundary of the stream
            if s == 0x0A and (p + n - 1) // SUB_BITS != (p - 1) // SUB_BITS and p > 0:
                cuts.add((-p) % SUB_BITS if p % SUB_BITS else 0)         # bits of the symbol in front of the boundary (0: it starts on it)
        ends = ends or any(e % SUB_BITS == 0 for e in st.block_end)
        out.append(st)
    assert cuts >= set(range(26)), sorted(cuts)
    assert ends
    return out


@functools.lru_cache(maxsize=None)
def periodic():
    """periodic streams, how a saturated region of a real frame looks, 20 or more lanes each: flat grey (period 11 bits), flat 4:2:0
    (an all-zero stream: ANY bit is a code boundary of some block phase), one repeated non-trivial block, a repeated 4:2:0 MCU.  A
    mis-phased lane may never re-align on its own, truth travels one lane per pass: whether such an image settles within
    NOPESAC_JPEG_SYNC_PASSES is an observation (docs/kernels.md), the coefficients and pixels are right either way."""
    out = []
    n = -(-20 * SUB_BITS // 11)
    side = int(np.ceil(np.sqrt(n)))
    c = zeros(8 * side, 8 * side, GRAY)
    c[0][..., 0] = 0
    out.append(write("periodic_flat_gray", c, 8 * side, 8 * side, GRAY, dc=(DCL,), ac=(ACL,), td=(0,), ta=(0,)))
    side = int(np.ceil(np.sqrt(20 * SUB_BITS / 24)))
    c = zeros(16 * side, 16 * side, S420)
    st = write("periodic_flat_420", c, 16 * side - 7, 16 * side - 3, S420)
    assert set(st.scan[:-1]) == {0}
    out.append(st)
    blk = np.zeros(64, np.int64)
    blk[[0, 1, 2, 5, 9, 20, 40, 63]] = [30, -5, 3, 1, -1, 2, 1, -1]
    c = zeros(8 * 24, 8 * 24, GRAY)
    c[0][...] = blk
    out.append(write("periodic_repeated_block", c, 8 * 24 - 1, 8 * 24 - 1, GRAY, dc=(DCK0,), ac=(AC0,), td=(0,), ta=(0,)))
    c = zeros(16 * 14, 16 * 14, S420)
    c[0][...] = blk
    c[1][..., [0, 1, 8]] = [-20, 2, 1]
    c[2][..., [0, 3]] = [25, -1]
    out.append(write("periodic_repeated_mcu_420", c, 16 * 14, 16 * 14 - 9, S420))
    for s in out:
        in_range(s)
        assert n_lanes(s) >= 20, (s.name, n_lanes(s))
    return out


# ---------------------------------------------------------------------------------------------------------------- IDCT families
QWIDE = np.array([256 + 11 * k for k in range(64)], np.int64)                 # 16-bit table, every entry above 255


def _gray_blocks(name, blocks, q=Q1, **kw):
    blocks = np.asarray(blocks, np.int64).reshape(-1, 64)
    n = len(blocks)
    bw = 16 if n % 16 == 0 else (8 if n % 8 == 0 else n)
    return write(name, [blocks.reshape(n // bw, bw, 64)], 8 * bw, 8 * (n // bw), GRAY, qt=(q,), dc=(DCK0,), ac=(AC16,), td=(0,), ta=(0,), tq=(0,), **kw)


@functools.lru_cache(maxsize=None)
def idct_single():
    """a single coefficient of each sign at each of the 64 zigzag positions, amplitudes 1, 255 and 1023 at q = 1 (128 blocks each):
    a slip in the de-zigzag table or in any one multiplier shows at its own position; coefficient +-1 through a 16-bit table with every
    entry above 255 (products 256 .. 949; written with Pq = 1 under SOF1)"""
    out = []
    for amp in (1, 255, 1023):
        b = np.zeros((128, 64), np.int64)
        for k in range(64):
            b[2 * k, k], b[2 * k + 1, k] = amp, -amp
        out.append(in_range(_gray_blocks("idct_single_%d" % amp, b)))
    b = np.zeros((128, 64), np.int64)
    for k in range(64):
        b[2 * k, k], b[2 * k + 1, k] = 1, -1
    out.append(in_range(_gray_blocks("idct_single_q16", b, QWIDE)))
    assert out[-1].data[out[-1].data.index(b"\xff\xdb") + 4] == 0x10 and b"\xff\xc1" in out[-1].data
    return out


@functools.lru_cache(maxsize=None)
def idct_zero_rows_columns():
    """blocks whose AC terms vanish in whole columns or rows (jidctint.c shortcuts those; the kernel does not: same numbers), and
    blocks that hold one row or one column only"""
    rng = _rng(12)
    nat = np.zeros((64, 8, 8), np.int64)
    for i in range(64):
        v = rng.integers(-60, 61, (8, 8))
        if i % 4 == 0:
            v[1:, :] = 0                                   # first row only: every column has zero AC
        elif i % 4 == 1:
            v[:, 1:] = 0                                   # first column only
        elif i % 4 == 2:
            v[1:, rng.integers(0, 8)] = 0
            v[1:, rng.integers(0, 8)] = 0
        else:
            v[rng.integers(1, 8), :] = 0
            v[:, rng.integers(1, 8)] = 0
        nat[i] = v
    zz = nat.reshape(64, 64)[:, ZIGZAG]
    zz[:, 0] = rng.integers(-300, 300, 64)
    return [in_range(_gray_blocks("idct_zero_rows_columns", zz))]


@functools.lru_cache(maxsize=None)
def idct_clamp():
    """samples that reach exactly 0 and 255 and go past them into the clamp on both sides, the pre-limit value inside [-512, 511]"""
    q = Q1.copy()
    q[0] = 4
    dcs = [-256, -255, -257, -258, -300, -511, -1023, -1016, 254, 253, 255, 256, 300, 511, 1020, 1016, 0, 1, -1, 2, -2, 3, -3, 128]
    b = np.zeros((len(dcs) * 2, 64), np.int64)
    b[:len(dcs), 0] = dcs
    b[len(dcs):, 0] = np.clip(dcs, -990, 990)
    b[len(dcs):, 1] = 40                                   # a ramp across the block: part of it inside the range, part clamped
    b[len(dcs):, 2] = -25
    st = in_range(_gray_blocks("idct_clamp", b, q))
    y = prelimit(st.coef[0], st.qt[0]) + 128
    assert (y == 0).any() and (y == 255).any() and (y < 0).any() and (y > 255).any() and y.min() <= -300 and y.max() >= 600
    return [st]


DENSE_Q, DENSE_AMP = 8, 15


def _dense(amp, n=64):
    rng = _rng(77)
    return rng.choice([-1, 1], (n, 64)) * amp


@functools.lru_cache(maxsize=None)
def idct_dense():
    """dense blocks (all 64 coefficients +-A at q = 8, fixed signs) at the largest A for which the oracle's pre-limit value stays in
    [-512, 511]: asserted here for A and refuted for A + 1"""
    st = in_range(_gray_blocks("idct_dense_%d" % DENSE_AMP, _dense(DENSE_AMP), Q1 * DENSE_Q))
    y = prelimit(_dense(DENSE_AMP + 1), Q1 * DENSE_Q)
    assert y.min() < -512 or y.max() > 511
    return [st]


@functools.lru_cache(maxsize=None)
def idct_wrap():
    """Dense blocks of +-32 at q = 8: the pre-limit value passes +-512.  jpeg_idct_kernel follows jidctint.c's range-limit table, which
    WRAPS modulo 1024 (as the oracle does); libjpeg-turbo's SIMD inverse DCT SATURATES, so Pillow differs by up to 255 here.  No
    conforming encoder reaches this region (its coefficients come from samples within 0 .. 255).  Compared with the oracle only; the
    CPU test asserts that Pillow differs, which pins the deviation."""
    st = _gray_blocks("idct_wrap_32", _dense(32), Q1 * 8, wrap=True)
    lo, hi = prelimit_range(st)
    assert lo < -512 and hi > 511
    return [st]


# ---------------------------------------------------------------------------------------------------------------- upsampling, colour
def _dc_for(sample):
    """DC coefficient (q = 1) of a flat block of that sample value: (dc + 4) >> 3 = sample - 128"""
    return 8 * (sample - 128) if sample < 255 else 1016


@functools.lru_cache(maxsize=None)
def upsample_sizes():
    """widths 1 .. 9 x heights 1 .. 5 for 4:4:4, 4:2:2 and 4:2:0: dw <= 2 replication, the first and last column rules, dh = 1 with
    both context rows clamped; W % 4 in {1, 2, 3}: a thread's four pixels cross a row end, the last thread takes the byte-wise tail;
    odd-sized images in one batch: 16-byte image offsets"""
    out = []
    for si, samp in enumerate((S444, S422, S420)):
        for W in range(1, 10):
            for H in range(1, 6):
                rng = _rng(1000 * si + 10 * W + H)
                c = [random_blocks(rng, s, n_ac=6, amp=30, dc_step=300, dc_lim=500) for s in grid(W, H, samp)]
                for a in c:
                    a[..., 1:3] = rng.integers(-60, 61, a[..., 1:3].shape)      # strong gradients: neighbouring chroma samples differ
                out.append(in_range(write("size_%dx%d_%dx%d" % (samp[0], samp[1], W, H), c, W, H, samp)))
    return out


YCC = (91881, -22554, -46802, 116130)                 # jdcolor.c: FIX(1.40200), -FIX(0.34414), -FIX(0.71414), FIX(1.77200) at 16 bits


def ycc(y, cb, cr, k=YCC):
    """jdcolor.c's conversion with the four constants as parameters (k = YCC: oracle.jpeg_oracle.ycc_to_rgb)"""
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    rgb = [y + ((k[0] * cr + 32768) >> 16), y + ((k[1] * cb + 32768 + k[2] * cr) >> 16), y + ((k[3] * cb + 32768) >> 16)]
    return np.clip(np.stack(rgb, -1), 0, 255).astype(np.uint8)


def constant_observable(i, d):
    """Does YCC[i] + d give another pixel than YCC[i] for ANY 8-bit Cb x Cr at Y = 0, 128 or 255?  One unit on a 16-bit constant moves
    a result only where the product sits within |chroma| / 65536 of a rounding step: 91881 +- 1 and 116130 + 1 change NOTHING on the
    whole domain (no test can tell them from the true constants), 116130 - 1 changes Cb = 3 and 253 (where B clamps unless Y is at the
    other end), the two G constants ~58 pairs each."""
    v = np.arange(256)
    cb, cr = np.meshgrid(v, v)
    k = list(YCC)
    k[i] += d
    return any(bool((ycc(np.full(cb.shape, y), cb, cr, k) != ycc(np.full(cb.shape, y), cb, cr)).any()) for y in (0, 128, 255))


@functools.lru_cache(maxsize=None)
def colour_values():
    """flat planes of Y in {0, 128, 255} x Cb, Cr in {0, 128, 255} (all 27, DC-only blocks: the clamps and every fixed-point term's
    rounding) in 4:4:4 and 4:2:0; 4:2:0 with chroma that alternates from sample to sample in both directions (all four triangle weights
    of h2v2 see different values) and 4:2:2 likewise; a 256 x 256 4:4:4 image that holds (nearly) every Cb x Cr pair, on which each of the
    four conversion constants, moved by one unit either way, changes a pixel wherever it changes any Cb x Cr pair at all (asserted here
    with the oracle's formula; 91881 +- 1 and 116130 + 1 change none)"""
    out = []
    assert [(_dc_for(s) + 4) >> 3 for s in (0, 128, 255)] == [-128, 0, 127]
    for samp in (S444, S420):
        for y in (0, 128, 255):
            for cb in (0, 128, 255):
                for cr in (0, 128, 255):
                    c = zeros(18, 17, samp)
                    for a, v in zip(c, (y, cb, cr)):
                        a[..., 0] = _dc_for(v)
                    st = in_range(write("flat_%dx%d_y%d_cb%d_cr%d" % (samp + (y, cb, cr)), c, 18, 17, samp))
                    px = [prelimit(cc, Q1) + 128 for cc in st.coef]
                    assert all(int(p.min()) == int(p.max()) == v for p, v in zip(px, (y, cb, cr)))
                    out.append(st)
    for samp, W, H in ((S420, 45, 37), (S422, 45, 19), (S420, 31, 33)):
        rng = _rng(W)
        c = zeros(W, H, samp)
        c[0][...] = random_blocks(rng, c[0].shape[:2], n_ac=5, amp=20)
        for a, amp in ((c[1], 230), (c[2], -200)):
            a[..., 63] = amp                               # the (7, 7) basis function: a checkerboard whose amplitude varies across the block
            a[..., 0] = rng.integers(-300, 300, a.shape[:2])
            a[..., 35] = 90
        out.append(in_range(write("checker_%dx%d_%dx%d" % (samp[0], samp[1], W, H), c, W, H, samp)))
    # 4:4:4, 256 x 256, Y flat at 0 / 128 / 255, Cb a ramp along x and Cr a ramp along y: (nearly) every Cb x Cr pair, nothing clamped: every
    # one-unit change of a conversion constant that is observable at all (constant_observable) moves a pixel of this image
    step = np.arange(32) * 64 - 996                        # block b of a ramp holds the samples 8 b .. 8 b + 7
    moved = {}
    for y in (0, 128, 255):
        c = zeros(256, 256, S444)
        c[0][..., 0] = _dc_for(y)
        c[1][..., 0], c[1][..., 1] = step[None, :], -20
        c[2][..., 0], c[2][..., 2] = step[:, None], -20
        st = in_range(write("chroma_plane_444_y%d" % y, c, 256, 256, S444))
        fr = J.parse(st.data)
        J.geometry(fr)
        pl = J.planes(fr, st.natural())
        assert np.array_equal(ycc(*pl), st.pixels()) and len(np.unique(pl[1])) >= 250 and len(np.unique(pl[2])) >= 250
        for i in range(4):
            for d in (-1, 1):
                k = list(YCC)
                k[i] += d
                moved[i, d] = moved.get((i, d), False) or bool((ycc(*pl, k=k) != st.pixels()).any())
        out.append(st)
    assert all(m == constant_observable(i, d) for (i, d), m in moved.items()), moved
    return out


# ---------------------------------------------------------------------------------------------------------------- the tables
ENTROPY = {"code_lengths": code_lengths, "one_symbol_tables": one_symbol_tables, "table_ids": table_ids, "categories": categories,
           "runs_and_block_ends": runs_and_block_ends, "dc_prediction": dc_prediction, "stuffing": stuffing,
           "restart_intervals": restart_intervals, "lane_thresholds": lane_thresholds, "lane_counts": lane_counts,
           "lane_boundary": lane_boundary, "periodic": periodic}
IDCT = {"idct_single": idct_single, "idct_zero_rows_columns": idct_zero_rows_columns, "idct_clamp": idct_clamp, "idct_dense": idct_dense,
        "idct_wrap": idct_wrap}
COLOUR = {"upsample_sizes": upsample_sizes, "colour_values": colour_values}
FAMILIES = {**ENTROPY, **IDCT, **COLOUR}


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """one batch in shuffled order: images for the lanes, images below the threshold, restart images, colour and grey, and one image
    the lanes give up on (periodic_flat_420: an all-zero 4:2:0 stream, every lane's guess of the block phase is self-consistent)"""
    pick = lane_thresholds() + [lane_counts()[2]] + restart_intervals()[:5] + [periodic()[1], periodic()[2]] + table_ids()[::5] + \
        dc_prediction()[1:] + stuffing()[::4] + upsample_sizes()[7::31] + [idct_clamp()[0], categories()[1]]
    order = _rng(5).permutation(len(pick))
    out = [pick[i] for i in order]
    assert sum(n_lanes(s) > 0 for s in out) >= 6 and sum(len(s.seg_bytes) > 1 for s in out) >= 5
    assert sum(n_lanes(s) == 0 and len(s.seg_bytes) == 1 for s in out) >= 6
    return out
