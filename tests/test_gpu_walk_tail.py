"""The two tails of walk_kernel<1> (zgpu_lz_walk.hip).  Behind a chunk's walkers the rest of the parse runs in one of two forms: the whole-chunk
form (zgpu_lz_tail.h: the games numbered in position order, their successors by number, the path threaded once through blocks of 64 games) when the
chunk's logs hold no more games than the table of successors has room for, and the windowed form (zgpu_lz_parse_body.inc with LOG) otherwise, or when the
whole-chunk threading's optimistic assumption did not hold.  ZGPU_WALK_TAIL_CAP, read at every launch, lowers the capacity; 0 sends every chunk
through the windowed form.

Every input goes through the default path in independent chunks of at most 64 KiB, in groups of at most 16 chunks a launch, with `last` 0 and 1, with
the default capacity AND with ZGPU_WALK_TAIL_CAP=0, and each result is compared byte for byte with the compiled reference where oracle/_ref is there
(the CPU restatement otherwise) and with LZ_SORTED, which shares none of this code: the windowed form stays tested now that it is the fallback.  A
release build cannot say which form ran; the inputs are built so that the interesting cases occur -- chunk lengths around a block of the threading and
around the former windows, logs of exactly as many games as a capacity, one fewer and one more, chunks over any capacity next to chunks under it, a
window in which the walkers' parses do not fall into step, games across former window edges -- and equality on both sides is the check.  The plain tests
at the end check on the CPU that the inputs are what they claim."""
import functools

import pytest

from oracle import cases, oracle_py as O, refzlib as R

gpu_test = pytest.mark.gpu

WIN, CHUNK = 8192, 65536
Z_FILTERED = 1
CONFIGS = {"L4": (4, 0), "L6": (6, 0), "L9": (9, 0), "L6-filtered": (6, Z_FILTERED)}
KINDS = ["text", "mix", "runs", "zeros", "period", "rand"]
LENGTHS = [1, 2, 3, 127, 128, 129, 8191, 8192, 8193, 65535, 65536]
ENV = "ZGPU_WALK_TAIL_CAP"


# ------------------------------------------------------------------ generators (the ones of tests/test_gpu_walk_end.py that are needed, restated)
def planted(n, seed):
    """n bytes to plant: pairs of bytes below and above 128, which neither cases.nomatch() (they alternate there) nor the text (all below) contains."""
    r = cases.make("rand", n, seed)
    return bytes((b & 0x7F) | (0x80 if (k >> 1) & 1 else 0) for k, b in enumerate(r))


def nomatch_windows(k):
    """k windows in which no three-byte string has an earlier copy within reach: cases.nomatch() repeats after 32768 bytes, beyond MAX_DIST."""
    return (cases.nomatch(32768) * 2)[: k * WIN]


def debruijn(k, n):
    """The lexicographically least de Bruijn sequence B(k, n) (Lyndon words): every n-gram once, every (n-1)-gram k times."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1: p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


@functools.lru_cache(maxsize=None)
def debruijn_bytes():
    return bytes(97 + v for v in debruijn(6, 6))


def debruijn_then_empty():
    """Five windows of B(6, 6) -- a five-byte match at every position, walkers that do not meet: logs that are full at level 9 -- and an empty one behind."""
    return debruijn_bytes()[: 5 * WIN] + nomatch_windows(1)


def no_meeting():
    """One window of B(6, 6) between two of text.  Its match tokens are five bytes long and mostly six positions apart (test_stride_is_what_it_claims):
    walkers started at different residues modulo six do not fall into step, the window's log is full, and a path whose games are six positions apart runs
    through the games of the other five residues without standing on them.  The chunk stays under the capacity: at most 8 192 games in the window,
    some 1 250 in each window of text."""
    return cases.make("text", WIN, 71) + debruijn_bytes()[:WIN] + cases.make("text", WIN + 5, 72)


def deferred(seed, first_k):
    """Text in which, at every former window edge e = 8192 w, a game starts k = 1, 2 or 3 positions in front of e (k cycling from first_k) and ends with a
    long match that starts AT e: at e - k + j (j < k) the longest match has 4 + j bytes, which the lazy evaluation gives up for the longer one a
    position further, and at e it has 203.  Returns (data, [(edge, k, distance of the match at the edge)])."""
    d = bytearray(cases.make("text", CHUNK, seed))
    claims = []
    for w in range(1, CHUNK // WIN):
        e, k = w * WIN, (first_k + w - 1) % 3 + 1
        T = planted(k + 3, seed * 100 + w) + planted(200, seed * 100 + 50 + w)   # the string at e - k; T[k:] is the long match at e
        at = e - 4000
        for j in range(k):                                                        # a copy of T[j: j + 4 + j], then a byte that differs
            d[at - 1] = 0xF0 + j
            d[at: at + 4 + j] = T[j: j + 4 + j]
            d[at + 4 + j] = T[j + 4 + j] ^ 0x3C
            at += 16
        d[at - 1] = 0xF8
        d[at: at + len(T) - k] = T[k:]
        d[at + len(T) - k] = 0xF9
        d[e - k - 1] = 0xFA
        d[e - k: e - k + len(T)] = T
        d[e - k + len(T)] = 0xFB
        claims.append((e, k, e - at))
    return bytes(d), claims


def counted(k_a, k_b):
    """Four windows (n = 32768: uniform blocks of 64): bytes without a match, window 1 with exactly k_a and window 3 with exactly k_b planted six-byte
    repeats, each a copy of six bytes of the (empty) window in front of it.  Eight repeats fill a block of 64 positions from its second position on,
    eight positions apart; the 1 025th comes from one block that holds nine, seven apart.  No block start lies inside a planted match, and where no
    byte has a match a walker goes from neutral position to neutral position until it stands on one that is claimed: every position is visited once,
    by the walker of its block, and every planted match is ONE game in the chunk's logs -- k_a + k_b games in all, which is what the capacity is
    compared with.  Returns (data, {window: [(position, distance)]})."""
    nm = cases.nomatch(32768)
    d, plants = bytearray(nm), {}
    for k, wsrc, wdst in ((k_a, 0, 1), (k_b, 2, 3)):
        base, cells = wdst * WIN, []
        if k > 1024:
            cells += [base + 64 + 1 + 7 * j for j in range(9)]
        for b in range(WIN // 64):
            if not (k > 1024 and b == 1):
                cells += [base + 64 * b + 2 + 8 * j for j in range(8)]
        cells = sorted(cells)[:k]
        assert len(cells) == k
        out = []
        for j, p in enumerate(cells):
            s = wsrc * WIN + 3 + 6 * j
            d[p: p + 6] = nm[s: s + 6]
            if p + 6 < len(d) and d[p + 6] == nm[s + 6]:   # (six bytes and no more, in front and behind)
                d[p + 6] ^= 1
            if d[p - 1] == nm[s - 1]:
                d[p - 1] ^= 1
            out.append((p, p - s))
        plants[wdst] = out
    return bytes(d), plants


# name -> (k_a, k_b, the capacities to run it with: its games, one fewer, one more)
BOUNDARIES = {"count-1-1023": (1, 1023, (1023, 1024, 1025)), "count-1024-1025": (1024, 1025, (2048, 2049, 2050))}


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> bytes, claims (name -> what the CPU tests check), groups (name -> names, at most 16 chunks a launch)."""
    ins, claims, groups = {}, {}, {}
    for kind in KINDS:
        for n in LENGTHS:
            ins["%s-%d" % (kind, n)] = cases.make(kind, n, 5)
    by_len = list(ins)
    for i in range(0, len(by_len), 16):
        groups["lengths-%d" % (i // 16)] = by_len[i: i + 16]
    for name, (ka, kb, _) in BOUNDARIES.items():
        ins[name], claims[name] = counted(ka, kb)
        groups[name] = [name]
    ins["debruijn-empty"] = debruijn_then_empty()
    ins["no-meeting"] = no_meeting()
    for i, (s, fk) in enumerate(((61, 0), (62, 1), (63, 2))):
        ins["deferred-%d" % i], claims["deferred-%d" % i] = deferred(s, fk)
    ins["text-24581"] = cases.make("text", 3 * WIN + 5, 6)
    # over any capacity (five full logs at level 9; a game at every other position of a run) next to chunks under it, in one launch
    groups["over-under"] = ["text-65536", "debruijn-empty", "mix-65536", "zeros-65536", "text-24581", "debruijn-empty", "mix-8193"]
    groups["no-meeting"] = ["no-meeting", "text-24581", "no-meeting"]
    groups["deferred"] = ["deferred-%d" % i for i in range(3)]
    # neighbouring workgroups in different tails at once: short, full, empty-log and over-capacity chunks side by side
    groups["sixteen"] = ["text-3", "zeros-65536", "mix-65536", "debruijn-empty", "rand-65536", "no-meeting", "count-1-1023", "text-129", "period-65536", "deferred-0",
                         "runs-65535", "count-1024-1025", "text-65536", "deferred-1", "mix-8191", "rand-1"]
    assert len(set(groups["sixteen"])) == 16
    assert all(1 <= len(g) <= 16 and all(n in ins and len(ins[n]) <= CHUNK for n in g) for g in groups.values())
    return ins, claims, groups


N_LENGTHS = (len(KINDS) * len(LENGTHS) + 15) // 16
GROUPS = ["lengths-%d" % i for i in range(N_LENGTHS)] + ["over-under", "no-meeting", "deferred", "sixteen"]
_ref_cache = {}


def reference(cfg, name, last):
    """The reference's raw chunk for one input (computed once per configuration and ending, shared by every test)."""
    key = (cfg, name, last)
    if key not in _ref_cache:
        level, strategy = CONFIGS[cfg]
        data = inputs()[0][name]
        _ref_cache[key] = R.deflate_chunk_raw(data, level, last, strategy=strategy) if R.available() else O.deflate_chunk(data, level, last, strategy=strategy)
    return _ref_cache[key]


@pytest.fixture(scope="module")
def eng():
    import zlib_amd
    e = zlib_amd.Engine(0)
    yield e
    e.close()


def check(eng, monkeypatch, cfg, names, caps):
    """The inputs in one launch, with `last` 0 and 1 and every capacity of `caps` (None: the default): each result against the reference and LZ_SORTED."""
    from zlib_amd import gpu
    ins = inputs()[0]
    level, strategy = CONFIGS[cfg]
    for last in (0, 1):
        flags = gpu.F_FINAL if last else 0
        want = [reference(cfg, n, bool(last)) for n in names]
        monkeypatch.delenv(ENV, raising=False)
        sorted_ = eng.deflate_segments_host([ins[n] for n in names], level, flags=flags, lz_impl=gpu.LZ_SORTED, strategy=strategy)
        for cap in caps:
            if cap is None:
                monkeypatch.delenv(ENV, raising=False)
            else:
                monkeypatch.setenv(ENV, str(cap))
            got = eng.deflate_segments_host([ins[n] for n in names], level, flags=flags, lz_impl=gpu.LZ_AUTO, strategy=strategy)
            for n, w, g, s in zip(names, want, got, sorted_):
                assert g == w, (cfg, n, last, cap, "default path differs from the reference", len(g), len(w))
                assert s == g, (cfg, n, last, cap, "default path differs from LZ_SORTED")


@gpu_test
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_both_tails(eng, monkeypatch, cfg, group):
    """Three-way parity: the default capacity, ZGPU_WALK_TAIL_CAP=0 (every chunk through the windowed tail), the reference."""
    check(eng, monkeypatch, cfg, inputs()[2][group], (None, 0))


@gpu_test
@pytest.mark.parametrize("name", list(BOUNDARIES))
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_capacity_boundary(eng, monkeypatch, cfg, name):
    """A chunk of exactly G games with a capacity of G - 1 (windowed), G and G + 1 (whole-chunk), and with the default and 0."""
    check(eng, monkeypatch, cfg, [name], BOUNDARIES[name][2] + (None, 0))


# ------------------------------------------------------------------ the inputs are what they claim (CPU restatement; no GPU)
def tokens_at(data, level=6):
    _, _, toks = O.deflate_chunk(data, level, True, want_tokens=True)
    pos, at = 0, {}
    for dist, lc in toks:
        at[pos] = (dist, lc)
        pos += lc + 3 if dist else 1
    return at


def matches_by_window(at):
    """Match tokens of the parse by the window they start in: each is the end of one game on the path."""
    c = [0] * (CHUNK // WIN)
    for p, (dist, _) in at.items():
        if dist:
            c[p // WIN] += 1
    return c


def test_groups_are_complete():
    ins, _, groups = inputs()
    assert set(groups) == set(GROUPS) | set(BOUNDARIES)
    assert {n for g in groups.values() for n in g} == set(ins)
    assert {len(ins["%s-%d" % (k, n)]) for k in KINDS for n in LENGTHS} == set(LENGTHS)


def test_counted_inputs_are_what_they_claim():
    """Exactly k_a and k_b match tokens -- the planted ones, six bytes each -- in windows 1 and 3, none elsewhere: with the argument of counted(), the
    chunk's logs hold k_a + k_b games, the middle one of the capacities the chunk is run with."""
    ins, claims, _ = inputs()
    for name, (ka, kb, caps) in BOUNDARIES.items():
        d, plants = ins[name], claims[name]
        assert len(d) == 4 * WIN and caps == (ka + kb - 1, ka + kb, ka + kb + 1)
        for level in (4, 6, 9):
            at = tokens_at(d, level)
            assert matches_by_window(at)[:4] == [0, ka, 0, kb], (name, level)
            for w, k in ((1, ka), (3, kb)):
                assert len(plants[w]) == k
                for p, dist in plants[w]:
                    assert at[p] == (dist, 6 - 3) and p // WIN == w, (name, level, p, at.get(p))
        for w in (1, 3):   # no block start (every 64th position: n <= 32768) inside a planted match: a walker that started there would log a game of its own
            for p, _ in plants[w]:
                assert not any(p < s < p + 6 for s in (p // 64 * 64, p // 64 * 64 + 64)), (name, p)


def test_stride_is_what_it_claims():
    """The de Bruijn window of `no-meeting`: its match tokens are five bytes long and, at levels 6 and 9, at least 1 300 of the gaps between them are
    exactly six positions -- no multiple of which is a block of the threading or a power of two."""
    d = inputs()[0]["no-meeting"]
    assert len(d) == 3 * WIN + 5
    for level in (6, 9):
        at = tokens_at(d, level)
        ms = sorted(p for p, (dist, _) in at.items() if dist and WIN <= p < 2 * WIN)
        gaps = [y - x for x, y in zip(ms, ms[1:])]
        assert len(ms) >= 1300 and sum(g == 6 for g in gaps) >= 1300, (level, len(ms), sum(g == 6 for g in gaps))
        assert sum(at[p][1] == 5 - 3 for p in ms) >= 1300, level
    at = tokens_at(d, 4)
    assert sum(1 for p, (dist, _) in at.items() if dist and WIN <= p < 2 * WIN) >= 1300


def test_deferred_inputs_are_what_they_claim():
    ins, claims, _ = inputs()
    seen = set()
    for i in range(3):
        d, cl = ins["deferred-%d" % i], claims["deferred-%d" % i]
        at = tokens_at(d)
        assert [e for e, _, _ in cl] == [w * WIN for w in range(1, 8)]
        for e, k, dist in cl:
            seen.add((e, k))
            for j in range(k):   # literals in front of the edge: the game that starts at e - k gives its matches up one by one
                assert at[e - k + j] == (0, d[e - k + j]), (i, e, k, j, at.get(e - k + j))
            assert at[e] == (dist, 203 - 3), (i, e, k, at.get(e))
    assert seen == {(w * WIN, k) for w in range(1, 8) for k in (1, 2, 3)}
