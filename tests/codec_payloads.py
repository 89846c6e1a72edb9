"""Adversarial payloads for the device block compressors (test infrastructure, plain helpers).

sdb_compress_blocks compresses a block as windows of 4 KiB, each on its own: matches never reach into an
earlier window, and every window is one deflate block / one zstd block / one run of lz4 or snappy elements.
The real SST blocks of the other tests all look alike, so each generator here aims at one branch of the
encoder and says which.  Every generator is deterministic (seeded); tests/test_codec_payloads.py asserts
the properties that belong to the input (Huffman depths, sizes, alphabets) on the CPU, and
tests/test_gpu_codec_write_edges.py asserts on the device's own streams that the branches ran.

payload_list() is the whole list as (name, bytes) pairs; blocks_of() frames it for sdb_compress_blocks
(a block is payload ++ 4 trailing bytes: the kernel does not read the stored CRC).
"""
import heapq

import numpy as np

WIN = 4096  # the compressor's window


def _rng(seed):
    return np.random.default_rng(seed)


def rand_bytes(n, seed, lo=0, hi=256):
    return _rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


def text(n, seed=1):
    """English-like key=value text: the compressible window (dynamic Huffman, FSE sequence tables)."""
    rng = _rng(seed)
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(120)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, 120))] + (b"=" if rng.integers(0, 4) == 0 else b" ")
    return bytes(out[:n])


# ---------------------------------------------------------------------------------------------------
# Huffman depth (the length limit of wave_huff_lengths)
# ---------------------------------------------------------------------------------------------------
def huffman_depth(freqs):
    """The longest code of a Huffman code for the nonzero counts, ties resolved toward the shallower tree
    (as the encoder's two-queue method does by preferring leaves): the least depth any optimal code has."""
    h = [(int(f), 0) for f in freqs if f]
    if len(h) < 2:
        return len(h)
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def min_total_for_depth(d):
    """The least total count of a histogram whose every Huffman code is d deep: counts 1, 1, 2, 3, 5, ...
    (d + 1 of them; anything smaller leaves a tie that the shallower tree wins)."""
    a, b, tot = 1, 1, 0
    for _ in range(d + 1):
        tot += a
        a, b = b, a + b
    return tot


def fibonacci_counts(k):
    c = [1, 1]
    while len(c) < k:
        c.append(c[-1] + c[-2])
    return c[:k]


def skewed(counts, symbols, shuffled, seed):
    """counts[i] copies of symbols[i]: sorted (runs of one byte: matches at offset 1 take all but a few
    literals) or shuffled (the frequent symbols form repeated 4-grams, the rare ones stay literals)."""
    b = np.concatenate([np.full(c, s, np.uint8) for c, s in zip(counts, symbols)])
    if shuffled:
        _rng(seed).shuffle(b)
    return b.tobytes()


def fibonacci_payload(k, shuffled, seed=3):
    """Fibonacci counts over k byte values: Huffman depth k - 1.  k = 18 (6764 bytes, two windows) has depth
    17 > 15, deflate's limit; k = 16 (2583 bytes) is the deepest that fits one window.  Target: the
    Kraft-sum fix of wave_huff_lengths (zstd's limit of 11 is within reach of one window; see
    deep_literals).

    Deflate's limit of 15 cannot be reached by this encoder, by construction: a deflate block codes one
    window, at most 4096 literals / lengths + the end-of-block symbol = 4097 symbols, and a histogram
    forces a code of depth 16 only from min_total_for_depth(16) = 4180 symbols on (below that a tie decides
    the depth, and the encoder's two-queue method takes the leaf on a tie, which gives the shallowest
    optimal tree).  The same holds for the distance code (at most 1024 matches).  So "a dynamic block with
    a 15-bit literal / length code" is not a witness the device streams can show; the CPU test pins the
    arithmetic, and the GPU test asserts its premise on every device stream (one deflate block per window,
    at most 4097 symbols in it).  The limit itself is witnessed at zstd's 11 bits (deep_literals,
    wide_skewed_payload) and at the code-length code's 7 (cl_limit_payload): the same function."""
    syms = list(range(65, 65 + k))
    return skewed(fibonacci_counts(k), syms, shuffled, seed)


def pow2_payload(shuffled, seed=4):
    """Counts 1, 1, 2, 4, ..., 2048 over 13 byte values: exactly one window, Huffman depth 12 > 11 (zstd's
    limit).  What reaches the literals section is what the matches leave over."""
    counts = [1] + [1 << i for i in range(12)]
    return skewed(counts, list(range(48, 48 + 13)), shuffled, seed)


def wide_skewed_payload(seed=5):
    """A skewed histogram over 224 byte values up to 255, shuffled, one window: zstd's tree description has
    only its FSE-compressed form (more than 128 weights cannot be written directly); when that form is
    refused the literals go raw."""
    rng = _rng(seed)
    syms = rng.permutation(256)[:224].astype(np.uint8)
    syms[0] = 255
    w = 0.97 ** np.arange(224)
    counts = np.maximum(1, np.floor(w / w.sum() * (WIN - 224))).astype(int)
    counts[0] += WIN - counts.sum()
    return skewed(counts, syms, True, seed)


# byte values per deflate code length: with counts 2048 >> length (and the end-of-block symbol as the second
# 11-bit code) the histogram is dyadic, so every Huffman code for it has exactly these lengths
CL_LENGTHS = {4: 3, 5: 5, 6: 8, 7: 13, 8: 21, 9: 150, 10: 55, 11: 1}


def cl_limit_code_lengths():
    """The code length of byte value 0, 1, ..., 255: the most frequent length that does not make a run of
    three equal lengths longer (deflate's code-length sequence codes longer runs as repeats)."""
    rem, out = dict(CL_LENGTHS), []
    while any(rem.values()):
        for n in sorted(rem, key=lambda n: -rem[n]):
            if rem[n] and not (len(out) >= 2 and out[-1] == out[-2] == n):
                out.append(n)
                rem[n] -= 1
                break
        else:
            raise ValueError("a run of equal lengths")
    return out


def cl_limit_payload(seed=0):
    """The length limit of deflate's code-length code (7 bits).  2047 bytes over all 256 values, value v
    2048 >> cl_limit_code_lengths()[v] times, in an order in which no 4 bytes repeat (no match: every byte
    a literal).  The literal / length code then has 3, 5, 8, 13, 21, 150, 55 and 2 codes of 4 .. 11 bits,
    its code-length sequence no run to repeat, and with the two 1-bit placeholder distance codes the
    code-length code's histogram is 2, 2, 3, 5, 8, 13, 21, 55, 150: a Huffman code 8 deep."""
    lens = cl_limit_code_lengths()
    b = np.concatenate([np.full(2048 >> n, v, np.uint8) for v, n in enumerate(lens)])

    def make(s):
        c = b.copy()
        _rng(s).shuffle(c)
        return c.tobytes()
    return _first(make, lambda p: len({p[i:i + 4] for i in range(len(p) - 3)}) == len(p) - 3, seed)


def distinct_3grams(k, length, seed):
    """`length` symbols below k, every 3-gram distinct, every symbol equally often (to within one): greedy,
    the least used symbol whose 3-gram is new."""
    rng = _rng(seed)
    seq, used, seen = [], [0] * k, set()
    for _ in range(length):
        for s in sorted(range(k), key=lambda s: (used[s], rng.random())):
            if len(seq) < 2 or (seq[-2], seq[-1], s) not in seen:
                break
        else:
            raise ValueError("no new 3-gram")
        if len(seq) >= 2:
            seen.add((seq[-2], seq[-1], s))
        seq.append(s)
        used[s] += 1
    return seq


DEEP_CHAIN = 13    # byte values 0..12 with counts 1, 1, 2, 3, 5, ..., 233
DEEP_MARKERS = 16  # byte values 16..31


def deep_literals(seed=6):
    """Literals whose histogram forces a Huffman code deeper than 11 (zstd's limit) in one window.  A
    skewed histogram alone does not do it: its frequent values repeat as 4-grams and leave as matches.  So
    each of the 609 chain literals (13 byte values, counts 1, 1, 2, 3, 5, ..., 233) stands alone between
    4-byte markers: the window starts with a dictionary of 612 bytes over 16 other values in which every
    3-gram is distinct (no match inside it), and literal i is followed by dictionary[j : j + 4] for a j of
    its own.  The 4 bytes from a chain literal on never repeat (its marker's first 3 bytes are its own), so
    no match covers it, and a marker's match ends at the next chain literal.  The literals section is the
    dictionary + the chain: deep_literal_counts()."""
    rng = _rng(seed)
    n = sum(fibonacci_counts(DEEP_CHAIN))
    d = bytes(16 + s for s in distinct_3grams(DEEP_MARKERS, n + 3, seed))
    chain = np.frombuffer(skewed(fibonacci_counts(DEEP_CHAIN), list(range(DEEP_CHAIN)), True, seed), np.uint8)
    out = bytearray(d)
    for x, j in zip(chain, rng.permutation(n)):
        out.append(int(x))
        out += d[j:j + 4]
    return bytes(out)


def deep_literal_counts():
    """The literal histogram of deep_literals() when every marker is found: the dictionary and the chain."""
    n = sum(fibonacci_counts(DEEP_CHAIN))
    d = np.bincount(np.asarray(distinct_3grams(DEEP_MARKERS, n + 3, 6)), minlength=DEEP_MARKERS)
    return fibonacci_counts(DEEP_CHAIN) + [int(c) for c in d]


# ---------------------------------------------------------------------------------------------------
# Window kinds and mixes (seams between windows)
# ---------------------------------------------------------------------------------------------------
def few_matches(n, seed, offsets=(1000, 2000)):
    """Uniform random bytes with a 4-byte repeat per offset: the window has sequences, but its compressed
    form is not smaller than the bytes, so zstd discards the attempt for a raw block and deflate stores."""
    b = bytearray(rand_bytes(n, seed))
    at = n - 600
    for off in offsets:
        if at - off >= 0 and at + 4 <= n:
            b[at:at + 4] = b[at - off:at - off + 4]
        at += 100
    return bytes(b)


def periodic(n, period, seed):
    """Random bytes repeated with one period: every match has the same offset (repeat-offset codes)."""
    p = rand_bytes(period, seed)
    return (p * (n // period + 1))[:n]


def window_kind(kind, n, seed):
    if kind == "text":
        return text(n, seed)
    if kind == "const":
        return bytes([seed & 0xFF]) * n
    if kind == "rand":
        return rand_bytes(n, seed)
    if kind == "rand4":
        return rand_bytes(n, seed, 100, 104)
    if kind == "rand16":
        return rand_bytes(n, seed, 32, 48)
    if kind == "few":
        return few_matches(n, seed)
    if kind == "periodic":
        return periodic(n, 700, 77)  # the same period and bytes wherever it stands
    raise ValueError(kind)


def window_mix(kinds, total, seed):
    """Windows of the given kinds in order (cycled) up to `total` bytes; the last one is cut short."""
    out = bytearray()
    i = 0
    while len(out) < total:
        out += window_kind(kinds[i % len(kinds)], min(WIN, total - len(out)), seed + i)
        i += 1
    return bytes(out)


MIX_SIZES = [4095, 4096, 4097, 8192, 12289, 65791, 65792, 65536 + 4]
MIX_ORDERS = [
    ("text", "const", "rand", "rand4", "rand16", "few"),
    ("rand", "text", "const", "few", "rand16", "rand4"),
    ("const", "few", "rand4", "text", "rand", "rand16"),
    ("rand16", "rand4", "few", "rand", "const", "text"),
]


def window_mixes():
    out = []
    for i, total in enumerate(MIX_SIZES):
        order = MIX_ORDERS[i % len(MIX_ORDERS)]
        out.append(("mix-%d-%s" % (total, order[0]), window_mix(order, total, 100 + 10 * i)))
    # compressible -> discarded attempt -> compressible with the first window's offset: the repeat offsets
    # of the discarded window must not leak into the third (zstd: rep[] carried across windows)
    out.append(("mix-rep-carry", window_mix(("periodic", "few", "periodic"), 3 * WIN, 200)))
    out.append(("mix-rep-carry-tail", window_mix(("periodic", "few", "periodic"), 2 * WIN + 1500, 210)))
    # stored -> dynamic -> a tiny last window (fixed Huffman): the deflate bit position carried across
    # windows, and every block kind in one stream
    out.append(("mix-stored-dynamic-fixed", window_mix(("rand", "text"), 2 * WIN, 220) + b"tiny last window!"))
    out.append(("mix-dynamic-stored-fixed", window_mix(("text", "rand"), 2 * WIN, 230) + b"abcabcabd"))
    # raw -> RLE -> compressed in one zstd frame, the constant window in the middle
    out.append(("mix-rand-const-text", window_mix(("rand", "const", "text"), 3 * WIN, 240)))
    # lz4: windows with no match at all (the one-lane literal-only fallback) and with matches only later
    out.append(("mix-rand-only-8k", rand_bytes(2 * WIN, 250)))
    out.append(("mix-text-rand", window_mix(("text", "rand", "text"), 3 * WIN - 7, 260)))
    # 17 incompressible windows: every codec at its literal-only worst case (17 stored deflate blocks, 17 raw
    # zstd blocks, one lz4 / snappy literal), the bound its slot counts on
    out.append(("mix-rand-only-64k", rand_bytes(65536 + 4, 270)))
    return out


# ---------------------------------------------------------------------------------------------------
# Sequence stress (element boundaries)
# ---------------------------------------------------------------------------------------------------
def grams_replay(seed=7):
    """455 distinct 4-grams, then the same 4-grams in shuffled order each followed by one fresh byte: one
    window of matches of exactly 4 bytes with one literal between them (the most sequences 4-byte matches
    with fresh sources allow: 4 N + 5 N <= 4096)."""
    rng = _rng(seed)
    n = 455
    # 4-grams over disjoint byte ranges per position in the gram, so that no 4 bytes across two grams repeat
    g = np.stack([rng.permutation(n) % 64 + 64 * j for j in range(4)], 1).astype(np.uint8)
    g[:, 3] = (np.arange(n) // 64 + 192 + 8 * (np.arange(n) % 8)).astype(np.uint8)  # (g0, g3) distinct
    g[:, 0] = (np.arange(n) % 64).astype(np.uint8)
    first = g.reshape(-1)
    order = rng.permutation(n)
    fresh = rng.integers(0, 256, n, dtype=np.uint8)
    second = np.concatenate([g[order], fresh[:, None]], 1).reshape(-1)
    return np.concatenate([first, second]).tobytes()


def grams_dictionary(seed=8):
    """A dictionary of 64 4-grams (256 bytes), then 960 of them in random order: one full window of about a
    thousand 4-byte sequences with no literals between them (kCzMaxSeq, 16 chunks of the element loop)."""
    rng = _rng(seed)
    g = np.stack([np.arange(64), rng.permutation(64) + 64, rng.permutation(64) + 128, rng.permutation(64) + 192], 1)
    g = g.astype(np.uint8)
    pick = rng.integers(0, 64, 960)
    return np.concatenate([g.reshape(-1), g[pick].reshape(-1)]).tobytes()


def cz_hash(p, i):
    """The compressor's hash of the 4 bytes at p[i:] (sdb_codec_enc.hip cz_hash: 11 bits)."""
    v = p[i] | p[i + 1] << 8 | p[i + 2] << 16 | p[i + 3] << 24
    return ((v * 2654435761) & 0xFFFFFFFF) >> 21


def single_probe_source(p, pos):
    """Where lz4 / snappy look for a match at pos: the latest earlier position with the same hash (they
    probe that one position, like lz4_flex / snap; zlib / zstd walk a chain).  None: no candidate."""
    h = cz_hash(p, pos)
    for q in range(pos - 1, -1, -1):
        if cz_hash(p, q) == h:
            return q
    return None


def _first(make, ok, seed):
    """make(seed), make(seed + 1), ...: the first that is ok (deterministic)."""
    for s in range(seed, seed + 400):
        p = make(s)
        if ok(p):
            return p
    raise ValueError("no seed in range")


def exact_match(length, seed):
    """300 random bytes, 20 more, then the first `length` of them again and a random tail: one match of
    exactly `length` bytes (lengths over 258 split at the window's maximum match).  No hash collision hides
    the source from the single-probe finders."""
    def make(s):
        src = rand_bytes(max(300, length), s)
        return src + rand_bytes(20, s + 1000) + src[:length] + rand_bytes(16, s + 2000)
    at = max(300, length) + 20
    return _first(make, lambda p: single_probe_source(p, at) == 0 and p[at + length] != p[length], seed)


MATCH_LENGTHS = [4, 18, 19, 258, 259, 273, 274, 275]


def literal_run(lit, seed):
    """`lit` literals, then a match: an 8-byte gram, random bytes, the gram again, and a random tail of 14
    bytes (long enough for lz4's end rules, short enough to need no length extension of its own)."""
    def make(s):
        g = rand_bytes(8, s)
        return g + rand_bytes(lit - 8, s + 1000) + g + rand_bytes(14, s + 2000)
    return _first(make, lambda p: single_probe_source(p, lit) == 0 and p[lit + 8] != p[8], seed)


LITERAL_RUNS = [14, 15, 16, 60, 61, 256, 257, 269, 270, 271, 4000]


def offset_match(off, seed, length=40):
    """One match of `length` bytes at distance `off` (1, 2, 3: a run of a 1-, 2-, 3-byte pattern), random
    around it."""
    if off <= 3:
        return rand_bytes(24, seed) + (rand_bytes(off, seed + 1) * 44)[:44] + rand_bytes(16, seed + 2)

    def make(s):
        p = rand_bytes(off, s)
        return p + p[:length] + rand_bytes(16, s + 2000)
    return _first(make, lambda p: single_probe_source(p, off) == 0 and p[off + length] != p[length], seed)


OFFSETS = [1, 2, 3, 2047, 2048, 4000]
SHORT_OFFSETS = [2047, 2048]  # 8-byte matches: snappy's copy-1 holds 4..11 bytes below offset 2048


def end_match(glen, tail, seed):
    """A gram of glen bytes, 30 random bytes, the gram again, then `tail` bytes to the end of the block: a
    match that would run into the last 12 / last 5 bytes (lz4's end rules drop it or clip it)."""
    def make(s):
        g = rand_bytes(glen, s)
        return g + rand_bytes(30, s + 1000) + g + rand_bytes(tail, s + 2000)
    at = glen + 30
    return _first(make, lambda p: single_probe_source(p, at) == 0 and (not tail or p[at + glen] != p[glen]), seed)


END_MATCHES = [(8, t) for t in (0, 1, 3, 4, 5, 6)] + [(16, t) for t in (0, 1, 4, 5, 6)]


def lz4_end_rule_length(glen, tail):
    """What lz4 may keep of end_match's match: it starts 12+ bytes before the end and ends 5+ before it."""
    at, n = glen + 30, 2 * glen + 30 + tail
    if at + 12 > n:
        return 0
    ln = min(glen, n - 5 - at)
    return ln if ln >= 4 else 0


LAZY_AT = 4 + 20 + 12 + 20  # the position of the 4-byte match; the 12-byte one starts one further


def lazy_match(seed=9):
    """A 4-byte match at q and a 12-byte match at q + 1: the parse must defer to the longer one."""
    def make(s):
        w = _rng(s).permutation(256)[:16].astype(np.uint8).tobytes()  # 16 distinct bytes
        s1 = w[0:4]                 # w x y z
        s2 = w[1:4] + w[4:13]       # x y z + 9 more
        return (s1 + rand_bytes(20, s + 1000, 0, 16) + s2 + rand_bytes(20, s + 2000, 16, 32)
                + w[0:4] + w[4:13] + rand_bytes(20, s + 3000, 32, 48))
    return _first(make, lambda p: single_probe_source(p, LAZY_AT) == 0 and single_probe_source(p, LAZY_AT + 1) == 24,
                  seed)


def sequence_stress():
    out = [("grams-replay", grams_replay()), ("grams-dictionary", grams_dictionary())]
    out += [("match-%d" % n, exact_match(n, 300 + n)) for n in MATCH_LENGTHS]
    out += [("litrun-%d" % n, literal_run(n, 4000 + n)) for n in LITERAL_RUNS]
    out += [("offset-%d" % n, offset_match(n, 5000 + n)) for n in OFFSETS]
    out += [("offset8-%d" % n, offset_match(n, 6000 + n, 8)) for n in SHORT_OFFSETS]
    out += [("endmatch-%d-%d" % (g, t), end_match(g, t, 7000 + 20 * g + t)) for g, t in END_MATCHES]
    out.append(("lazy", lazy_match()))
    return out


# ---------------------------------------------------------------------------------------------------
# Degenerate sizes and alphabets
# ---------------------------------------------------------------------------------------------------
DEGENERATE_LENGTHS = [0, 1, 2, 3, 4, 5, 12, 13, 15, 16, 63, 64, 65, 127, 128, 255, 256, 16383, 16384]


def degenerate():
    t = text(16384, 11)
    out = [("len-%d" % n, t[:n]) for n in DEGENERATE_LENGTHS]
    out += [("rand-%d" % n, rand_bytes(n, 700 + n)) for n in (1, 5, 16, 64, 255, 256)]
    # 300 consecutive blocks of 0..6 bytes: tiny adjacent slots
    out += [("tiny-%03d" % k, rand_bytes(k % 7, 800 + k)) for k in range(300)]
    out += [("one-symbol-%d" % n, b"\xa5" * n) for n in (1, 15, 16, 300, WIN, WIN + 904)]
    out.append(("two-symbols-random", rand_bytes(1000, 12, 7, 9)))
    out.append(("two-symbols-alternating", b"\x00\xff" * 700))
    out.append(("two-symbols-rare", b"\x11" * 2000 + b"\x22" + b"\x11" * 2000))
    return out


def skewed_histograms():
    return [
        ("fib18-sorted", fibonacci_payload(18, False)), ("fib18-shuffled", fibonacci_payload(18, True)),
        ("fib16-sorted", fibonacci_payload(16, False)), ("fib16-shuffled", fibonacci_payload(16, True)),
        ("pow2-sorted", pow2_payload(False)), ("pow2-shuffled", pow2_payload(True)),
        ("wide-skewed", wide_skewed_payload()), ("deep-literals", deep_literals()),
        ("cl-limit", cl_limit_payload()),
        ("small-alphabet-200", rand_bytes(200, 13, 32, 48)),   # < 256 literals: one Huffman stream
        ("small-alphabet-900", rand_bytes(900, 14, 32, 48)),   # 4 streams, the 3-byte literals header
        ("small-alphabet-low", rand_bytes(900, 16, 0, 9)),     # byte values 0..8: direct weights are shortest
        ("random-then-copy", rand_bytes(2048, 15) * 2),        # raw literals inside a compressed block
    ]


def payload_list():
    """Every payload as (name, bytes): a few hundred KiB, one compress launch per codec."""
    return skewed_histograms() + window_mixes() + sequence_stress() + degenerate()


def blocks_of(payloads):
    """The list framed for sdb_compress_blocks: (data uint8 array, block offsets uint64): payload ++ 4
    trailing bytes per block (the kernel does not read them)."""
    parts, off = [], [0]
    for _, p in payloads:
        parts.append(bytes(p) + b"\xde\xad\xbe\xef")
        off.append(off[-1] + len(p) + 4)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(off, np.uint64)
