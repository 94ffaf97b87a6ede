"""Helpers of the dynamic-Huffman PNG tests, independent of the C++:

  parse_blocks      walks the deflate blocks of a concatenated IDAT stream by hand (fixed, dynamic and empty stored blocks)
  huffman_optimum   the heap construction: the optimal cost sum f * depth and the least depth an optimal tree can have
  fixed_price / dynamic_price   the exact bits of a token list as either block type, the header rule of include/dvd_hip.h
                    restated (lengths come from the caller)
  CASES             the seeded images both the CPU and the GPU tests encode
"""
import heapq
import os
import struct

import numpy as np

import png_model as P

ROOT = P.ROOT
S = P.header_segment()
GOLDEN = os.path.join(ROOT, "tests", "golden")
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


# ---- the block parser ---------------------------------------------------------------------------------------------------------
class _Reader:
    def __init__(self, data, pos=0):
        self.data, self.pos = data, pos                    # pos in bits

    def bits(self, n):                                     # LSB first; n <= 16
        at = self.pos >> 3
        v = (int.from_bytes(self.data[at:at + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)
        self.pos += n
        return v

    def symbol(self, table):                               # a Huffman code: MSB first, so bit-reversed in the stream
        at = self.pos >> 3
        entry = table[(int.from_bytes(self.data[at:at + 3], "little") >> (self.pos & 7)) & 0x7FFF]
        assert entry >= 0, "no code of up to 15 bits matches"
        self.pos += entry & 15
        return entry >> 4


def canonical(lengths):
    """The codes of RFC 1951 section 3.2.2 as a decoding table: the next 15 bits of the stream -> symbol << 4 | length, -1
    where no code matches (an incomplete code)."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    table = np.full(1 << 15, -1, np.int64)
    for sym, n in enumerate(lengths):
        if n:
            assert nxt[n] < 1 << n, "the code is over-subscribed"
            table[int(format(nxt[n], f"0{n}b")[::-1], 2)::1 << n] = sym << 4 | n
            nxt[n] += 1
    return table.tolist()


def kraft(lengths):
    """(sum of 2^-len over the used symbols) as an exact fraction of 2^15."""
    return sum(1 << (15 - n) for n in lengths if n)


def parse_blocks(idat):
    """The blocks of a zlib stream: a list of dicts with type ('fixed' | 'dynamic' | 'stored'), final, bits (the block's whole
    length, for a stored block with its padding), tokens (literals as int, matches as (length, distance)) and, for a dynamic
    block, ll_len / d_len / cl_len (code lengths by symbol, HLIT / HDIST / 19 long), hlit, hdist, hclen, header_bits.  The four
    bytes behind the final block are the Adler-32."""
    r = _Reader(idat, 16)
    blocks = []
    while True:
        start = r.pos
        final, kind = r.bits(1), r.bits(2)
        blk = {"final": final, "tokens": []}
        if kind == 0:
            r.pos = (r.pos + 7) & ~7
            n, nn = r.bits(16), r.bits(16)
            assert n == 0 and nn == 0xFFFF, "only the empty stored block is part of the format"
            blk["type"] = "stored"
        else:
            assert kind in (1, 2)
            if kind == 1:
                blk["type"] = "fixed"
                ll, dd = canonical(FIXED_LL), canonical([5] * 30)
            else:
                blk["type"] = "dynamic"
                hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
                cl_len = [0] * 19
                for k in range(hclen):
                    cl_len[CL_ORDER[k]] = r.bits(3)
                cl = canonical(cl_len)
                lens = []
                while len(lens) < hlit + hdist:
                    sym = r.symbol(cl)
                    if sym < 16:
                        lens.append(sym)
                    elif sym == 16:
                        lens += [lens[-1]] * (3 + r.bits(2))
                    elif sym == 17:
                        lens += [0] * (3 + r.bits(3))
                    else:
                        lens += [0] * (11 + r.bits(7))
                assert len(lens) == hlit + hdist, "a run crosses out of the concatenated lengths"
                blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_len=cl_len, ll_len=lens[:hlit], d_len=lens[hlit:],
                           header_bits=r.pos - start - 3)
                ll, dd = canonical(lens[:hlit]), canonical(lens[hlit:])
            while True:
                sym = r.symbol(ll)
                if sym < 256:
                    blk["tokens"].append(sym)
                elif sym == 256:
                    break
                else:
                    assert sym <= 285
                    length = LEN_BASE[sym - 257] + r.bits(LEN_EXTRA[sym - 257])
                    d = r.symbol(dd)
                    assert d < 30
                    blk["tokens"].append((length, DIST_BASE[d] + r.bits(DIST_EXTRA[d])))
        blk["bits"] = r.pos - start
        blocks.append(blk)
        if final:
            break
    assert (r.pos + 7) // 8 + 4 == len(idat), "the Adler-32 does not follow the final block"
    return blocks


def idat_of(data):
    """The concatenated IDAT data of a PNG file."""
    pos, out = 8, b""
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IDAT":
            out += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    return out


# ---- pricing ------------------------------------------------------------------------------------------------------------------
def len_symbol(length):
    sym = max(k for k in range(29) if LEN_BASE[k] <= length) if length < 258 else 28
    return 257 + sym, LEN_EXTRA[sym]


def dist_symbol(dist):
    sym = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return sym, DIST_EXTRA[sym]


def histograms(tokens):
    """([286] literal/length counts with one end-of-block, [30] distance counts, extra bits of all matches)."""
    ll, dd, extra = [0] * 286, [0] * 30, 0
    ll[256] = 1
    for t in tokens:
        if isinstance(t, tuple):
            s, e = len_symbol(t[0])
            d, de = dist_symbol(t[1])
            ll[s] += 1
            dd[d] += 1
            extra += e + de
        else:
            ll[t] += 1
    return ll, dd, extra


def fixed_price(tokens):
    ll, dd, extra = histograms(tokens)
    return 3 + sum(f * n for f, n in zip(ll, FIXED_LL)) + 5 * sum(dd) + extra


def rle_symbols(lens):
    """The greedy run-length coding of the concatenated lengths: [(symbol, extra bits)]."""
    out, i = [], 0
    while i < len(lens):
        v, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                c = min(run, 138)
                out.append((18, 7))
                run -= c
            if run >= 3:
                out.append((17, 3))
                run = 0
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                out.append((16, 2))
                run -= min(run, 6)
        out += [(v, 0)] * run
    return out


def dynamic_price(tokens, code_lengths):
    """The bits of `tokens` as one dynamic block under the header rule.  code_lengths(freq, limit) -> lengths is the builder
    under test (the host program's --code-lengths)."""
    ll, dd, extra = histograms(tokens)
    ll_len, d_len = code_lengths(ll, 15), code_lengths(dd, 15)
    hlit = max(257, max(k + 1 for k in range(286) if ll_len[k]))
    hdist = max([1] + [k + 1 for k in range(30) if d_len[k]])
    rle = rle_symbols(ll_len[:hlit] + d_len[:hdist])
    cl_freq = [0] * 19
    for sym, _ in rle:
        cl_freq[sym] += 1
    cl_len = code_lengths(cl_freq, 7)
    if sum(1 for n in cl_len if n) == 1:
        cl_len[18 if cl_len[0] else 0] = 1
    hclen = max(4, max(k + 1 for k in range(19) if cl_len[CL_ORDER[k]]))
    header = 14 + 3 * hclen + sum(cl_len[sym] + e for sym, e in rle)
    return 3 + header + sum(f * n for f, n in zip(ll, ll_len)) + sum(f * n for f, n in zip(dd, d_len)) + extra


# ---- the Huffman optimum ------------------------------------------------------------------------------------------------------
def huffman_optimum(freq):
    """(cost, depth) of an optimal prefix code of the non-zero entries of freq: cost = sum f * length; depth = the greatest
    length of the optimal code whose greatest length is least (ties in the heap go to the shallower subtree).  One symbol: (f,
    1), the length the format gives it; none: (0, 0)."""
    used = [f for f in freq if f]
    if len(used) < 2:
        return (used[0], 1) if used else (0, 0)
    heap = [(f, 0, k) for k, f in enumerate(used)]
    heapq.heapify(heap)
    cost, serial = 0, len(used)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, serial))
        serial += 1
    return cost, heap[0][1]


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _rand(h, w, seed=0, hi=256):
    return np.random.RandomState(seed).randint(0, hi, (h, w, 3)).astype(np.uint8)


def _stream_shape(nbytes):
    """(h, w) with h * (3w + 1) == nbytes, the widest such image."""
    for w in range((nbytes - 1) // 3, 0, -1):
        if nbytes % (3 * w + 1) == 0:
            return nbytes // (3 * w + 1), w
    raise AssertionError(nbytes)


def _of_stream(n, seed):
    h, w = _stream_shape(n)
    return _rand(h, w, seed=seed, hi=4)               # few values: matches of every length


def _page(h=700, w=500):
    from benchmarks.png_time import page_image
    return page_image(h, w)


DEEP_RARE, DEEP_BYTES, DEEP_SEED = 11, 30000, 0


def deep_image(seed=DEEP_SEED, rare=DEEP_RARE, nbytes=DEEP_BYTES):
    """One row whose Sub residuals are a chosen stream of `nbytes` bytes (one segment): `rare` byte values 64, 65, ... with the
    counts 1 2 3 5 8 ... 144 (with the end-of-block's 1 a Fibonacci chain of 12 symbols, 11 deep) and, for the rest, the 128
    small residuals -64 .. 63 drawn uniformly (some 230 of each, so the chain's 376 hang six or seven levels down); pixel i =
    pixel i - 3 + residual.  The seeded order is mended so that no three bytes occur twice: the tokeniser finds no match,
    every byte stays a literal and the histogram is the chosen one.  Small residuals make Sub the cheapest filter."""
    rng = np.random.RandomState(seed)
    fib = [1, 2]
    while len(fib) < rare:
        fib.append(fib[-1] + fib[-2])
    tail = np.concatenate([np.full(f, 64 + k, np.uint8) for k, f in enumerate(fib)])
    bulk = (rng.randint(0, 128, nbytes - len(tail)) - 64).astype(np.uint8)
    res = np.concatenate([tail, bulk])
    assert len(res) % 3 == 0 and len(res) + 1 <= S
    rng.shuffle(res)
    res = res.tolist()
    seen = {(1, res[0], res[1])}                      # the stream starts with the filter byte 1
    for i in range(2, len(res)):
        for _ in range(100):
            if (res[i - 2], res[i - 1], res[i]) not in seen:
                break
            j = int(rng.randint(i, len(res)))
            res[i], res[j] = res[j], res[i]
        seen.add((res[i - 2], res[i - 1], res[i]))
    res = np.array(res, np.uint8)
    img = np.cumsum(res.reshape(-1, 3).astype(np.int64), axis=0) % 256
    return np.ascontiguousarray(img.astype(np.uint8)[None])


CASES = {
    "1x1": lambda: _rand(1, 1, 1), "1x7": lambda: _rand(1, 7, 2), "7x1": lambda: _rand(7, 1, 3), "2x2": lambda: _rand(2, 2, 4),
    "stream_S-1": lambda: _of_stream(S - 1, 5), "stream_S": lambda: _of_stream(S, 6), "stream_S+1": lambda: _of_stream(S + 1, 7),
    "period5": lambda: (np.arange(200 * 333 * 3) % 5 * 50).astype(np.uint8).reshape(200, 333, 3),
    "zeros_256": lambda: np.zeros((256, 256, 3), np.uint8),
    "random_97x131": lambda: _rand(97, 131, 9),
    "7_segments_200x333": lambda: _rand(200, 333, 8, hi=16),
    "page_700x500": _page,
    "deep": deep_image,
}
# For the digests alone (the block parser above would take minutes on its 5 MB): a stream of 2731 * 3073 bytes = 257 segments of
# 32 KiB, so that a lane of png_layout_kernel's scan owns more than one segment.
LARGE_CASES = {"257_segments_2731x1024": lambda: _page(2731, 1024)}
DIGEST_CASES = {**CASES, **LARGE_CASES}
_cache = {}


def case(name):
    """The image of a case, made once and never changed (read-only)."""
    if name not in _cache:
        img = np.ascontiguousarray(DIGEST_CASES[name]())
        img.setflags(write=False)
        _cache[name] = img
    return _cache[name]
