"""Inputs of uneven shape for the combining extraction (tests/test_gpu_combine_ragged.py; validated on the CPU by
tests/test_ragged_inputs.py): reads of every length class around K and around the item cut, with N, lower case and empty
reads; records of many tiles with their edges on tile edges; tandem repeats; k-mers with more than 2^16 copies; and, for the EXTENSION payloads
(tests/test_gpu_ext_ragged.py), tiles crowded with read offsets around the scan's read-index window and runs of empty reads (crowded_index); for the
certain drops (tests/test_gpu_certain_drops.py), runs of one base inside reads and exact numbers of homopolymer k-mers (homopolymer_runs, homopolymer_edge).  Plain
functions, seeded and deterministic; every builder returns a list of strings (DnaBuffer.from_sequences / oracle.pack_reads
take it; pack() below gives the same arrays in one numpy pass)."""
import numpy as np

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")
_CODE = np.zeros(256, dtype=np.uint8)
for _ch, _c in (("C", 1), ("c", 1), ("G", 2), ("g", 2), ("T", 3), ("t", 3)):      # A, a, N, n -> 0 (DnaSeq::compress)
    _CODE[ord(_ch)] = _c


def item_cut(K):
    """k-mers per item of the combining extraction at most (ParseArgs::item_maxk): 16, or 61 - K for two-word keys (keys the plan does not take: 1)"""
    return max(1, min(16, 61 - K))


def revcomp(s):
    return s.translate(_COMP)[::-1]


def random_seq(rng, n):
    return _ACGT[rng.integers(0, 4, size=n, dtype=np.uint8)].tobytes().decode()


def pack(seqs):
    """(packed, read_off, read_len) of the reads, every read on a byte boundary: what oracle.pack_reads gives, in one pass"""
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    nb = (lens + 3) // 4
    off = np.zeros(len(seqs), dtype=np.int64)
    if len(seqs):
        off[1:] = np.cumsum(nb)[:-1]
    raw = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    first = np.zeros(len(seqs), dtype=np.int64)
    if len(seqs):
        first[1:] = np.cumsum(lens)[:-1]
    at = np.arange(raw.size, dtype=np.int64) + np.repeat(off * 4 - first, lens)      # base i of read r -> position 4 off[r] + i
    codes = np.zeros(int(nb.sum()) * 4, dtype=np.uint8)
    codes[at] = _CODE[raw]
    c = codes.reshape(-1, 4)
    packed = (c[:, 0] << 6) | (c[:, 1] << 4) | (c[:, 2] << 2) | c[:, 3]
    return np.ascontiguousarray(packed, dtype=np.uint8), off.astype(np.uint64), lens.astype(np.uint32)


def ragged_lengths(K):
    """the length classes of ragged(): none, one base, around K (all four len % 4 packing phases), supermers of one k-mer under the item cut,
    exactly the cut and one over it, the usual 150 and reads of four tiles' length"""
    kc = item_cut(K)
    return [0, 1, K - 1, K, K + 1, K + 2, K + 3, kc - 1 + K - 1, kc + K - 1, kc + K, 150, 2047, 2048, 2049]


def ragged(K, seed, nreads=6000, genome=60000):
    """`nreads` reads cut from a random genome on both strands, their lengths taken in turn from ragged_lengths(K); one read in twenty carries an N,
    one in twenty is lower case; the first and the last read are empty, and so is every fourteenth between them"""
    rng = np.random.default_rng([seed, K, 1])
    g = random_seq(rng, genome)
    classes = ragged_lengths(K)
    out = []
    for i in range(nreads):
        n = classes[i % len(classes)]
        at = int(rng.integers(0, genome - n + 1))
        s = g[at:at + n]
        if rng.integers(0, 2):
            s = revcomp(s)
        what = int(rng.integers(0, 20))
        if what == 0 and n:
            j = int(rng.integers(0, n))
            s = s[:j] + "N" + s[j + 1:]
        elif what == 1:
            s = s.lower()
        out.append(s)
    out.append("")
    return out


def long_records(K, seed, variant=0):
    """test_long_records_and_tile_edges at a fifth of its size: a record of 2048 x 150 bases that ends on a parse tile edge (the next one starts on
    it), a 200 kbp record, a record shorter than K, a slice of the first record (counts of 2) and a last record after which the packed buffer ends
    exactly on a tile edge (variant 0) or two bytes behind a whole word (variant 1: the tail branch of the placement's word staging)"""
    rng = np.random.default_rng([seed, K, 2])
    a = random_seq(rng, 2048 * 150)
    reads = [a, random_seq(rng, 200000), random_seq(rng, K - 1), a[1000:60000]]
    pre = sum((len(r) + 3) // 4 for r in reads)
    reads.append(random_seq(rng, 4 * ((-pre) % 512 + 1024) + (5 if variant else 0)))
    return reads


def tandem_periods(K):
    return [1, 2, 3, 5, K - 1, K, K + 1]


def low_complexity_reads(K, seed):
    """the tandem repeats of low_complexity() alone: ~40 reads of 150-400 bases per period; period 1: 25 poly-A and 25 poly-T reads of 150 bases
    (one canonical k-mer across strands, 50 x (151 - K) copies) besides poly-C and poly-G; even K: reads whose unit is its own reverse complement"""
    rng = np.random.default_rng([seed, K, 3])
    out = []
    for p in tandem_periods(K):
        if p == 1:
            out += ["A" * 150] * 25 + ["T" * 150] * 25
            out += [b * int(rng.integers(150, 401)) for b in "CG" for _ in range(8)]
            continue
        for _ in range(40):
            unit = random_seq(rng, p)
            n = int(rng.integers(150, 401))
            out.append((unit * (n // p + 1))[:n])
    if K % 2 == 0:
        for _ in range(10):
            half = random_seq(rng, K // 2)
            unit = half + revcomp(half)                        # a k-mer that is its own reverse complement, once per period
            n = int(rng.integers(150, 401))
            out.append((unit * (n // K + 1))[:n])
            out.append(random_seq(rng, 7) + unit + random_seq(rng, 9))
    return out


def low_complexity(K, seed):
    """low_complexity_reads() shuffled into 2000 ragged reads"""
    rng = np.random.default_rng([seed, K, 4])
    reads = low_complexity_reads(K, seed) + ragged(K, seed, nreads=2000)
    return [reads[i] for i in rng.permutation(len(reads))]


PAST_16_COPIES = (65535, 65536, 65536 + 20, 2 * 65536 + 17)


def past_16_bits_kmers(K, seed):
    """the four k-mers of past_16_bits(), distinct as canonical k-mers"""
    rng = np.random.default_rng([seed, K, 5])
    while True:
        ks = [random_seq(rng, K) for _ in range(4)]
        if len({min(s, revcomp(s)) for s in ks}) == 4:
            return ks


def past_16_bits(K, seed, apart=True):
    """four k-mers as reads of exactly K bases (either strand), 65535, 65536, 65536 + 20 and 2 x 65536 + 17 copies, shuffled into 3000 ragged reads:
    the copies spread over many tiles and workgroups.  No background read holds one of the four (asserted; apart=False leaves that open: at K = 5 the
    background holds every k-mer there is, and the four only grow)."""
    rng = np.random.default_rng([seed, K, 6])
    ks = past_16_bits_kmers(K, seed)
    back = ragged(K, seed, nreads=3000)
    for s in back if apart else ():
        u = s.upper().replace("N", "A")                      # (as the reads are packed)
        assert not any(x in u or revcomp(x) in u for x in ks), "the background holds one of the four k-mers"
    pool = back + [x for x in ks for _ in (0, 1)]
    for j in range(4):
        pool[len(back) + 2 * j + 1] = revcomp(ks[j])
    idx = [np.arange(len(back), dtype=np.int64)]
    for j, n in enumerate(PAST_16_COPIES):
        idx.append(len(back) + 2 * j + (rng.integers(0, 2, size=n, dtype=np.int64)))
    idx = np.concatenate(idx)
    return [pool[i] for i in rng.permutation(idx)]


INDEX_TILE = 512            # bytes of the packed buffer per parse tile (PARSE_TILE / 4)
INDEX_WINDOW = 64           # read-index entries scan_kernel looks at per tile (PARSE_RWIN)
CROWDED_COUNTS = (62, 63, 64, 65, 66)
CROWDED_RUN = 100           # empty reads in a row


def crowded_index(K, seed, genome=8000):
    """~100 kbases for the read index of the EXTENSION payloads (the k-mers and counts of this input do not depend on it, every (pos, rid) does).
    Every read with k-mers is cut from one genome of 8000 bases, on both strands, so most k-mers occur in several reads.  In turn:
    100 empty reads in front of the first read with k-mers; 100 reads of 150 bases; for n = 62 ... 66 two tiles with exactly n read offsets
    inside their 512 bytes (empty reads and reads of 1-4 bases, one of K bases; the last of them a read that runs past the tile's end) -- one
    whose first read starts on the tile's first byte, the last read early in the tile, one whose first bytes belong to the read before, the last
    read starting 3 bytes before the tile's end; a tile of 451 offsets (reads of 1-4 bases and empty ones); 100 empty reads in front of a read
    of K bases; a record of three tiles and 40 bytes, behind it 70 reads of at most 4 bases and a read with k-mers in the same tile; reads of
    K ... K+3 bases in threes with an empty and a one-base read, in every order; reads with N and lower case; 100 empty reads.
    tests/test_ragged_inputs.py asserts all of it from pack()'s offsets."""
    rng = np.random.default_rng([seed, K, 7])
    g = random_seq(rng, genome)
    out, at_byte = [], [0]
    extra = (K + 3) // 4 + 1                                   # bytes past a tile's end that make a read of at least K bases

    def add(s):
        out.append(s)
        at_byte[0] += (len(s) + 3) // 4

    def cut(n):
        at = int(rng.integers(0, genome - n + 1))
        s = g[at:at + n]
        return revcomp(s) if rng.integers(0, 2) else s

    def tiny():
        return random_seq(rng, int(rng.integers(1, 5)))

    def fill_to(b):                                            # one read with k-mers that starts in one tile and ends in front of byte b of a later one
        need = (b - at_byte[0]) % INDEX_TILE
        if need <= b or 4 * need < K:
            need += INDEX_TILE
        add(cut(4 * need))

    def shorts(n, with_k):                                     # n reads of one byte at most; with_k: one of them has K bases instead
        for i in range(n):
            if with_k and i == n // 2:
                add(cut(K))
            else:
                add("" if i % 3 == 1 else tiny())

    def past_the_edge():                                       # the last read that starts in this tile: it ends `extra` bytes into the next one
        nb = INDEX_TILE - at_byte[0] % INDEX_TILE + extra
        add(cut(4 * nb - int(rng.integers(0, 4))))

    for _ in range(CROWDED_RUN):
        add("")
    add(cut(K + 2))
    for _ in range(100):
        add(cut(150))
    for n in CROWDED_COUNTS:
        fill_to(0)
        shorts(n - 1, True)
        past_the_edge()
        fill_to(5)
        shorts(n - 2, True)
        add(cut(4 * (INDEX_TILE - at_byte[0] % INDEX_TILE - 3)))
        past_the_edge()
    fill_to(0)
    shorts(450, False)
    past_the_edge()
    for _ in range(CROWDED_RUN):
        add("")
    add(cut(K))
    fill_to(0)
    add(cut(3 * 4 * INDEX_TILE + 160))
    shorts(70, False)
    past_the_edge()
    for _ in range(2):
        for p in range(4):
            three = ["", random_seq(rng, 1), None]
            for order in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
                for j in order:
                    add(cut(K + p) if three[j] is None else three[j])
    for _ in range(20):
        s = cut(150)
        j = int(rng.integers(0, 150))
        add(s[:j] + "N" + s[j + 1:])
        add(cut(150).lower())
    for _ in range(CROWDED_RUN):
        add("")
    return out


_BASES = "ACGT"
HOMO_SIZES = (1, 2, 63, 64, 65, 120, 200, 2048)      # copies per run of homopolymer_edge(): one, around a lane span of the sketch (64 positions), a tile
HOMO_DMIN = 1 << 16                                  # the sketch drops a homopolymer k-mer from max(U, 2^16) + 1 copies inside its sample on


def as_packed(s):
    """the read as the library sees it: upper case, N as A"""
    return s.upper().replace("N", "A")


def base_runs(seqs):
    """(read, start, length, code) of every maximal run of one base in the reads as they are packed (N and lower case mapped), as four int64 arrays"""
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    codes = _CODE[np.frombuffer("".join(seqs).encode(), dtype=np.uint8)]
    first = np.concatenate(([0], np.cumsum(lens)))
    read = np.repeat(np.arange(len(seqs), dtype=np.int64), lens)
    cut = np.ones(codes.size + 1, dtype=bool)
    if codes.size:
        cut[1:-1] = (codes[1:] != codes[:-1]) | (read[1:] != read[:-1])
    at = np.flatnonzero(cut)
    start, n = at[:-1], np.diff(at)
    return read[start], start - first[read[start]], n, codes[start].astype(np.int64)


def homopolymer_positions(seqs, K):
    """(all, sample): per base the number of positions whose forward k-mer is a homopolymer of it, as dicts {"A": n, "C": n, "G": n, "T": n} --
    over all reads, and over the reads before the last (the plan's sketch of an input below 4 MB of packed reads)"""
    read, _, n, code = base_runs(seqs)
    copies = np.maximum(n - K + 1, 0)
    out = []
    for sel in (np.ones(read.size, dtype=bool), read < len(seqs) - 1):
        out.append({b: int(copies[sel & (code == c)].sum()) for c, b in enumerate(_BASES)})
    return tuple(out)


def expected_drops(seqs, K, U):
    """(mask, dropped k-mer instances) of a call on these reads: bit 0 / 1 where the sample holds more than max(U, 2^16) copies of the all-A / the
    all-C k-mer (A + T, C + G runs); every position of such a k-mer, in all reads, is then left out"""
    every, sample = homopolymer_positions(seqs, K)
    dmin = max(U, HOMO_DMIN)
    mask = (1 if sample["A"] + sample["T"] > dmin else 0) | (2 if sample["C"] + sample["G"] > dmin else 0)
    return mask, (every["A"] + every["T"] if mask & 1 else 0) + (every["C"] + every["G"] if mask & 2 else 0)


def _other(rng, b):
    return _BASES[(_BASES.index(b) + int(rng.integers(1, 4))) % 4]


def _put_run(rng, s, at, n, b):
    """s with a run of exactly n bases b at `at`: the bases next to it are made to differ from b"""
    out = list(s)
    out[at:at + n] = b * n
    if at > 0 and as_packed(out[at - 1]) == b:
        out[at - 1] = _other(rng, b)
    if at + n < len(out) and as_packed(out[at + n]) == b:
        out[at + n] = _other(rng, b)
    return "".join(out)


HOMO_WHICH = ("AT", "CG", "both", "AT_over")
HOMO_GRID = [(31, 17), (32, 17), (33, 17), (51, 17), (56, 17), (57, 25), (21, 11), (11, 7), (5, 3)]      # K <= 32 / K > 32 arms of the scan's test, 57: the last K the mask serves
HOMO_NO_DROP_GRID = [(58, 17), (31, 26)]             # K beyond the mask's reach; M = SCAN_MAX_M + 1: the general parse kernels
HOMO_UNIFORM_GRID = [(31, 17), (51, 17), (33, 17)]
HOMO_EDGE_K = (31, 32, 33, 51, 57)
HOMO_REFUSED_K = (32,)                               # hsk_init takes no K that is a multiple of 32 (undefined in the reference): the builders and the oracle do, the GPU cases cannot
HOMO_INTERIOR = (-1, 0, 1, 7, 8, 9)                  # interior runs of K + d bases
HOMO_PATTERNS = ("whole", "from_start", "to_end") + tuple("interior%+d" % d for d in HOMO_INTERIOR) + ("two_runs", "then_complement", "a_then_c", "n_and_lower")


def _run_read(rng, K, s, pattern, b):
    """the background read s (at least 2 K + 3 bases) with the runs of `pattern` in base b"""
    n = len(s)
    comp = revcomp(b)
    if pattern == "whole":
        return b * n
    if pattern == "from_start":
        return _put_run(rng, s, 0, int(rng.integers(K, n - 9)), b)
    if pattern == "to_end":
        m = int(rng.integers(K, n - 9))
        return _put_run(rng, s, n - m, m, b)
    if pattern.startswith("interior"):
        m = K + int(pattern[8:])
        return _put_run(rng, s, int(rng.integers(1, n - m)), m, b)
    if pattern == "two_runs":                                      # b^m1 x b^m2: no k-mer holds the x and is a homopolymer
        room = n - 2 * K - 3
        m1 = K + int(rng.integers(0, room // 2 + 1)); m2 = K + int(rng.integers(0, room // 2 + 1))
        at = int(rng.integers(1, n - m1 - m2 - 1))
        s = _put_run(rng, s, at, m1, b)
        return _put_run(rng, s, at + m1 + 1, m2, b)
    if pattern in ("then_complement", "a_then_c"):                 # two runs back to back: no k-mer across the junction is a homopolymer
        second = comp if pattern == "then_complement" else _BASES[(_BASES.index(b) + 1) % 4]
        room = n - 2 * K - 2
        m1 = K + int(rng.integers(0, room // 2 + 1)); m2 = K + int(rng.integers(0, room // 2 + 1))
        at = int(rng.integers(1, n - m1 - m2))
        s = _put_run(rng, s, at + m1, m2, second)
        return _put_run(rng, s, at, m1, b)
    if pattern == "n_and_lower":                                   # A: an N and a lower-case stretch inside the run (both pack as A); other bases: lower case
        m = int(rng.integers(K + 8, n - 2))
        at = int(rng.integers(1, n - m))
        s = list(_put_run(rng, s, at, m, b))
        j = at + int(rng.integers(1, m - 6))
        s[j:j + 5] = b.lower() * 5
        if b == "A":
            s[at + int(rng.integers(0, m))] = "N"
        return "".join(s)
    raise ValueError(pattern)


def homopolymer_runs(K, seed, which, uniform=False, nreads=6000, genome=40000, long_record=True, reach=True):
    """~1 Mbp for the certain drops (tests/test_gpu_certain_drops.py): `nreads` reads cut from a random genome on both strands, K + 40 ... 260 bases
    long (uniform: all 150 bases), of which two in three carry runs of one base, the patterns of HOMO_PATTERNS in turn -- the whole read, a run
    from position 0, a run to the last base, interior runs of K - 1 ... K + 9 bases, two runs one base apart, a run followed by a run of the
    complement or of the next base, a run with an N and lower case inside.  `which` says which runs there are and which reach the sketch's threshold of
    2^16 + 1 copies inside the sample (whole-read runs are added until they do): "AT", "CG" (runs of these bases only), "both", "AT_over" (A / T
    reach it; C / G runs stop at ~10 000 copies: the all-C k-mer belongs in a U = 65535 list).  One record of 100 kbp with interior runs (not with
    uniform); the reads are shuffled; the last read is random and holds no run of K bases."""
    rng = np.random.default_rng([seed, K, 8, HOMO_WHICH.index(which), int(uniform)])
    g = random_seq(rng, genome)
    need = 2 * K + 4

    def cut(n):
        at = int(rng.integers(0, genome - n + 1))
        s = g[at:at + n]
        return revcomp(s) if rng.integers(0, 2) else s

    def length():
        return 150 if uniform else max(int(rng.integers(K + 40, 261)), need)

    full = {"AT": "AT", "CG": "CG", "both": "ACGT", "AT_over": "AT"}[which]
    few = "CG" if which == "AT_over" else ""
    few_copies = 0

    def add_run_read(b, pattern):
        if pattern == "a_then_c" and which in ("AT", "CG"):
            pattern = "then_complement"                            # (one family only: no run of the other)
        out.append(_run_read(rng, K, cut(length()), pattern, b))

    out = []
    turn = 0
    for i in range(nreads):
        if i % 3 == 2:
            out.append(cut(length()))
            continue
        pattern = HOMO_PATTERNS[turn % len(HOMO_PATTERNS)]
        bases = full
        if few and turn % 5 == 4 and few_copies < 10000:           # (13 patterns, every fifth turn: each pattern comes round)
            bases = few
        b = bases[(turn // len(HOMO_PATTERNS)) % len(bases)]
        add_run_read(b, pattern)
        if bases == few:
            got = homopolymer_positions([out[-1], ""], K)[0]
            few_copies += sum(got[x] for x in few)
        turn += 1
    # whole-read runs until every family that has to reach the threshold holds 2^16 + 1000 copies
    fams = {"AT": ["AT"], "CG": ["CG"], "both": ["AT", "CG"], "AT_over": ["AT"]}[which]
    have = homopolymer_positions(out + [""], K)[0]
    for fam in fams if reach else ():                              # (reach=False: the patterns alone, for a rank whose sketch is not the one that decides)
        n, j = have[fam[0]] + have[fam[1]], 0
        while n < HOMO_DMIN + 1000:
            m = length()
            out.append(fam[j % 2] * m)
            n += m - K + 1; j += 1
    order = rng.permutation(len(out))
    out = [out[i] for i in order]
    if long_record and not uniform:                                # positions beyond 2^16 for the payloads: interior runs every ~1500 bases
        rec = random_seq(rng, 100000)
        bases = full + few
        for j, at in enumerate(range(700, 99000, 1500)):
            rec = _put_run(rng, rec, at + int(rng.integers(0, 300)), K + HOMO_INTERIOR[j % len(HOMO_INTERIOR)] + (20 if j % 7 == 3 else 0), bases[j % len(bases)])
        out.insert(len(out) // 2, rec)
    while True:                                                    # the last read is outside the sketch's sample: it holds no run
        last = random_seq(rng, 150)
        if not any(b * K in last for b in _BASES):
            break
    out.append(last)
    return out


def _edge_pieces(copies):
    """`copies` as a sum of HOMO_SIZES taken in turn, the remainder in the largest sizes that still fit"""
    out, left, i = [], copies, 0
    while left >= HOMO_SIZES[i % len(HOMO_SIZES)] and left > sum(HOMO_SIZES):
        out.append(HOMO_SIZES[i % len(HOMO_SIZES)]); left -= out[-1]; i += 1
    for n in sorted(HOMO_SIZES, reverse=True):
        while left >= n:
            out.append(n); left -= n
    return out


def homopolymer_edge(K, seed, copies, base, single_run=False, nback=4500):
    """~0.3 Mbp with EXACTLY `copies` positions whose k-mer is a homopolymer of `base` or of its complement (in turn): runs of 1, 2, 63, 64, 65, 120,
    200 and 2048 copies (a run of c copies is c + K - 1 bases) between flanks of 0 - 12 random bases that do not extend them -- single_run: all
    copies in one record -- shuffled into `nback` random reads of K - 3 ... 90 bases, some of them shorter than K, none with a k-mer of one
    base.  The last read is one of the random reads."""
    rng = np.random.default_rng([seed, K, 9, copies, _BASES.index(base), int(single_run)])
    pieces = [copies] if single_run else _edge_pieces(copies)
    assert sum(pieces) == copies
    out = []
    for j, c in enumerate(pieces):
        b = revcomp(base) if j % 2 else base
        left, right = random_seq(rng, int(rng.integers(0, 13))), random_seq(rng, int(rng.integers(0, 13)))
        if left and left[-1] == b:
            left = left[:-1] + _other(rng, b)
        if right and right[0] == b:
            right = _other(rng, b) + right[1:]
        out.append(left + b * (c + K - 1) + right)
    back = []
    while len(back) < nback + 1:
        s = random_seq(rng, int(rng.integers(K - 3, 91)))
        if not any(b * K in s for b in _BASES):
            back.append(s)
    pool = out + back[:-1]
    return [pool[i] for i in rng.permutation(len(pool))] + [back[-1]]


def tiled(arrays, reps):
    """(packed, read_off, read_len) of `reps` copies of an input, one behind the other"""
    packed, off, lens = arrays
    offs = (off[None, :] + (np.arange(reps, dtype=np.uint64) * np.uint64(packed.size))[:, None]).reshape(-1)
    return np.tile(packed, reps), np.ascontiguousarray(offs, dtype=np.uint64), np.tile(lens, reps)


# the (K, M) grid of the tests: one-word keys -- (30, 15): even K, palindromes; (31, 25): the scan's largest M, a window of 7; (27, 5): a wide window,
# the 16-k-mer cut all the time -- and two-word keys -- (40, 17): the smallest K the plan takes; (45, 17): items of exactly 16 k-mers; (55, 23): of 6
GRID_ONE_WORD = [(31, 17), (21, 11), (30, 15), (16, 9), (13, 7), (31, 25), (27, 5)]
GRID_TWO_WORDS = [(40, 17), (42, 21), (45, 17), (51, 17), (55, 23)]
GRID = GRID_ONE_WORD + GRID_TWO_WORDS
SEED = 2024
