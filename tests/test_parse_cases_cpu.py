"""The match-search catalogue (oracle/parsecases.py) on the CPU: the restatement (oracle/deflate_oracle.c) gives the compiled reference's bytes
(tests/golden/parse_kat.json) for every case and configuration, the deflateTune rows included; every case is what it claims -- the token at
each probe is the claimed one, the two sides of a threshold get different tokens, no filler trigram lies in a bucket of the scenario."""
import hashlib

import numpy as np
import pytest

from oracle import oracle_py as O, parsecases as P, refzlib as R


def h16(b):
    return hashlib.sha256(b).hexdigest()[:16]


@pytest.fixture(scope="module")
def cat():
    return P.catalogue()


@pytest.fixture(scope="module")
def gold(golden):
    return golden("parse_kat.json")["cases"]


def chunk(c, cfg, last, want_tokens=False):
    k = P.CONFIGS[cfg]
    return O.deflate_chunk(c.data, k.level, bool(last), pos0_matchable=bool(k.p0), want_tokens=want_tokens, strategy=k.strategy, tune=k.tune)


_tokens = {}


def tokens_at(c, cfg, cont=None):
    """{position: token} of the restatement's parse (of the chunk, or of the one continuous stream), token = (dist, len) or LIT."""
    cont = c.cont if cont is None else cont
    if (c.name, cfg, cont) not in _tokens:
        k = P.CONFIGS[cfg]
        if cont:
            _, t = O.deflate_cont_tokens(c.data, k.level, k.strategy, tune=k.tune)
            dist, lc = t["dist"].astype(np.int64), t["lc"].astype(np.int64)
        else:
            _, _, toks = chunk(c, cfg, True, want_tokens=True)
            dist, lc = (np.array([t[j] for t in toks], dtype=np.int64) for j in (0, 1))
        step = np.where(dist > 0, lc + 3, 1)
        start = np.cumsum(step) - step
        assert int(step.sum()) == len(c.data)
        at = {}
        for pos, _ in c.claims[cfg]:  # (only the probes are looked up)
            i = int(np.searchsorted(start, pos))
            if i < len(start) and start[i] == pos:
                at[pos] = (int(dist[i]), int(lc[i]) + 3) if dist[i] else P.LIT
        _tokens[(c.name, cfg, cont)] = at
    return _tokens[(c.name, cfg, cont)]


def cont_bytes(c, cfg):
    k = P.CONFIGS[cfg]
    return O.deflate_cont_tokens(c.data, k.level, k.strategy, tune=k.tune)[0] if k.tune else O.deflate_cont(c.data, k.level)


def test_catalogue_is_the_one_the_golden_file_names(cat, gold):
    assert sorted(c.name for c in cat) == sorted(gold)
    for c in cat:
        assert gold[c.name]["data"] == [len(c.data), h16(c.data)], c.name
        assert sorted(gold[c.name]["out"]) == sorted(c.cfgs), c.name


def test_restatement_gives_the_golden_bytes(cat, gold):
    bad = []
    for c in cat:
        for cfg in c.cfgs:
            want = gold[c.name]["out"][cfg]
            if c.cont:
                z = cont_bytes(c, cfg)
                got = [len(z), h16(z)]
            else:
                zs = [chunk(c, cfg, last) for last in (0, 1)]
                got = [[len(z), h16(z)] for z in zs]
            if got != want:
                bad.append((c.name, cfg, got, want))
            if cfg in gold[c.name].get("cont", {}):
                z = cont_bytes(c, cfg)
                if [len(z), h16(z)] != gold[c.name]["cont"][cfg]:
                    bad.append((c.name, cfg, "continuous", len(z)))
    assert not bad, (len(bad), bad[:8])


def test_every_case_is_what_it_claims(cat, gold):
    """The token at every probe, read from the restatement's parse: of the chunk, of the continuous stream for the cases on a tile edge
    (ora_deflate_cont_tokens), and of both for the placed cases that go through both."""
    bad, ncont = [], 0
    for c in cat:
        for cfg in c.cfgs:
            for cont in [c.cont] + ([True] if cfg in gold[c.name].get("cont", {}) else []):
                at = tokens_at(c, cfg, cont)
                ncont += cont
                for pos, tok in c.claims[cfg]:
                    if at.get(pos) != tok:
                        bad.append((c.name, cfg, "cont" if cont else "chunk", pos, tok, at.get(pos)))
    assert not bad, (len(bad), bad[:8])
    assert ncont >= 9 * 12 * 2 + 3 * 12 * 2


def test_threshold_pairs_differ_across_the_threshold(cat):
    """The two sides of a pair: different tokens at the probe (chunk cases and continuous ones alike, from the restatement's own tokens), so a
    kernel off by one cannot pass both."""
    groups = {}
    for c in cat:
        if c.pair:
            groups.setdefault(c.pair[0], {}).setdefault(c.pair[1], []).append(c)
    assert len(groups) > 100
    for g, sides in groups.items():
        assert sorted(sides) == [0, 1], g
        a, b = sides[0][0], sides[1][0]
        assert a.cfgs == b.cfgs, g
        for cfg in a.cfgs:
            ta = [tokens_at(a, cfg).get(p) for p, _ in a.claims[cfg]]
            tb = [tokens_at(b, cfg).get(p) for p, _ in b.claims[cfg]]
            assert ta[0] != tb[0] and [t for _, t in a.claims[cfg]][0] != [t for _, t in b.claims[cfg]][0], (g, cfg, ta, tb)


def test_filler_keeps_out_of_the_scenarios_buckets(cat):
    """Every trigram that holds a filler byte occurs once in its input and falls into no bucket of a probe: nothing but the scenario's own
    strings is ever a candidate of a probe's chain."""
    for c in cat:
        a = np.frombuffer(c.data, dtype=np.uint8).astype(np.int64)
        f = c.fill
        code = (a[:-2] << 16) | (a[1:-1] << 8) | a[2:]
        anyf = f[:-2] | f[1:-1] | f[2:]
        _, inv, cnt = np.unique(code, return_inverse=True, return_counts=True)
        assert not (anyf & (cnt[inv] > 1)).any(), c.name
        assert c.buckets and not (anyf & np.isin(P.buckets_at(c.data), sorted(c.buckets))).any(), c.name
        assert (a[f] < 192).all() and (a[~f] >= 192).all(), c.name


def test_families_and_rows_the_catalogue_must_hold(cat):
    fam = {c.family for c in cat}
    assert fam == {"chain", "quarter", "nice", "clip", "tie", "stairs", "lazy", "short", "reach", "fast", "placed", "hand"}
    names = {c.name for c in cat}
    for cfg in P.FAST + P.SLOW:
        chain = P.row(cfg)[3]
        for d in (chain - 1, chain, chain + 1):
            assert {"chain-%s-%s-d%d" % (cfg, fl, d) for fl in ("tri", "bkt")} <= names
    assert P.row("T13")[3] >> 2 == 3 and P.row("T100")[3] >> 2 == 25 and P.row("T33")[3] == 33
    assert not any(c.family == "quarter" and c.cfgs == ["L4"] for c in cat)  # (good_length == max_lazy: unreachable, see parsecases)
    assert all(len(c.data) <= 65536 for c in cat if not c.cont)
    assert max(len(c.data) for c in cat if c.family == "chain" and c.cfgs == ["L9"]) < 26000
    # every claimed position of a continuous case lies on a tile edge; the cases with a match in hand (quarter, hand) claim the probe on the edge and the one
    # or two positions behind it, where the search that matters runs
    edges = set()
    for c in cat:
        if c.cont:
            claimed = sorted({p for cfg in c.cfgs for p, _ in c.claims[cfg]})
            assert claimed == list(range(claimed[0], claimed[-1] + 1)) and len(claimed) <= (3 if c.name.startswith(("hand-", "quarter-")) else 1), c.name
            edges.add(claimed[0])
    assert edges == {65023, 65024, 65025, 97535, 97536, 97537}


def test_rows_no_levels_row_resembles(cat, gold):
    """The deflateTune rows of parsecases.EDGE_SLOW / EDGE_FAST: each breaks the relation it is there for, the ladders are as deep as they say ON THE
    FINISHED BYTES (chain_of), an unbounded search finds the prize behind more decoys than any budget of the row, and the rows that go through one
    continuous stream have their cases on every tile edge and, a second time, on the block and window edges."""
    rows = {k: P.row(k) for k in list(P.EDGE_SLOW) + list(P.EDGE_FAST)}
    levels = set(P.ROWS.values())
    assert not set(rows.values()) & levels
    assert all(rows[k][3] >> 2 == 0 and rows[k][3] for k in ("Q3", "Q2", "Q1", "Q3-L4", "Q3-L9")) and rows["U0"][3] == 0 and rows["U70000"][3] > 0xffff
    assert all(rows[k][1] > rows[k][2] for k in ("LN258", "LN64")) and not any(g[1] > g[2] for g in levels)
    assert [rows[k][0] for k in ("G0", "G2", "G3", "G300")] == [0, 2, 3, 300] and [rows[k][1] for k in ("Z0", "Z2", "Z3")] == [0, 2, 3]
    assert [rows[k][2] for k in ("N0", "N2", "N3", "N1000")] == [0, 2, 3, 1000]
    assert {rows[k][1] - rows[k][2] for k in ("I0", "I3", "I7", "I8", "I258")} == {-8, -5, -1, 0, 250} and P.CONFIGS["I7"].level == 1 and P.CONFIGS["I31-L3"].level == 3
    assert P.budget("FG2") == 1 and P.budget("FG2U") == P.INF and P.budget("G2") == 32 and P.budget("G3") == 32 and P.budget("G3", 3) == 8 and P.budget("G300", 15) == 32
    by = {c.name: c for c in cat}
    deep = 0
    for c in cat:
        cfg = c.cfgs[0]
        if cfg not in rows or len(c.cfgs) != 1:
            continue
        good, lazy, nice, chain = rows[cfg]
        if c.name.startswith("chain-"):           # chain-<cfg>-<flavour>-d<depth>[-<tag>]: the prize is candidate number d of the probe
            d = int(c.name.split("-d")[1].split("-")[0])
            (probe, tok), = c.claims[cfg]
            ch = P.chain_of(c.data, probe)
            assert len(ch) == d and len(ch) <= max(40, P.DEEP), c.name
            assert (tok != P.LIT and tok[1] == 20 and probe - tok[0] == ch[d - 1]) == (d <= P.budget(cfg)), c.name
            deep += d == P.DEEP
        elif c.name.startswith("quarter-"):        # quarter-<cfg>-g<in hand>-d<depth>[-<tag>]: searched one position behind the probe, g bytes in hand
            g_, d = int(c.name.split("-g")[1].split("-")[0]), int(c.name.split("-d")[1].split("-")[0])
            q = c.claims[cfg][0][0]
            ch = P.chain_of(c.data, q + 1)
            assert len(ch) in (d, d + 1) and d <= max(40, P.DEEP), c.name  # (+ 1: the held copy's own second position, behind the prize)
            found = len(c.claims[cfg]) == 2 and c.claims[cfg][1][1][1] >= 20 and q + 1 - c.claims[cfg][1][1][0] == ch[d - 1]
            assert found == (d <= P.budget(cfg, g_)), c.name
            deep += d == P.DEEP
    assert deep == 2 * 2 + 2 * 2 + 5 + 1   # U0 / U70000: two ladders and two quarters each; one quarter per max_chain 1..3 row; FG2U
    for cfg, c in (("Q3", 3), ("Q2", 2), ("Q1", 1), ("Q3-L4", 3), ("Q3-L9", 3)):
        good = rows[cfg][0]
        assert {"quarter-%s-g%d-d%d" % (cfg, good, d) for d in (c + 1, 8, 40, P.DEEP)} | {"quarter-%s-g%d-d%d" % (cfg, good - 1, d) for d in (c, c + 1)} <= set(by)
        assert all(len(by["quarter-%s-g%d-d%d" % (cfg, good, d)].claims[cfg]) == 2 for d in (c + 1, 8, 40, P.DEEP)), cfg  # FOUND, however deep
        assert len(by["quarter-%s-g%d-d%d" % (cfg, good - 1, c + 1)].claims[cfg]) == 1, cfg                                 # one past max_chain: not found
    assert "quarter-Q3-g4-d%d" % P.DEEP in by and "chain-U0-bkt-d%d" % P.DEEP in by and "chain-FG2U-bkt-d%d" % P.DEEP in by
    # max_lazy <= 2: all literals where level 6 finds the repeats
    c = by["lazy-none-repeats"]
    for cfg in ("Z0", "Z2"):
        toks = chunk(c, cfg, True, want_tokens=True)[2]
        assert len(toks) == len(c.data) and all(t[0] == 0 for t in toks), cfg
    assert any(t[0] for t in chunk(c, "L6", True, want_tokens=True)[2])
    # max_lazy > nice_length: every case has nice_length <= h < max_lazy; the hole cases share nice_length bytes or more AND the two quick-check bytes
    hands = [c for c in cat if c.name.startswith("hand-")]
    assert sum("-hole" in c.name for c in hands) >= 4 and sum(c.pair is not None for c in hands) >= 8
    for c in hands:
        cfg = c.cfgs[0]
        h = int(c.name.split("-h")[1].split("-")[0])
        assert rows[cfg][2] <= h < rows[cfg][1], c.name
    # the continuous rows: every tile edge, and the block / window edge cases a second time
    for cfg in P.CONT_EDGE:
        tiles = [c for c in cat if c.cont and c.cfgs == [cfg]]
        assert {c.name.rsplit("-t", 1)[1] for c in tiles} == {"65023", "65024", "65025", "97535", "97536", "97537"}, cfg
        again = [c for c in cat if not c.cont and c.cfgs == [cfg] and cfg in gold[c.name].get("cont", {})]
        assert len(again) >= 12 and {c.name[-3] for c in again} == {"b", "w"}, cfg  # (-b-1, -b+0, ... -w+1)
    assert not any(c.cont and P.is_fast(cfg) and P.CONFIGS[cfg].tune for c in cat for cfg in c.cfgs)  # (tuned deflate_fast: chunks only)


def test_filler_helper():
    z = P.filler(70000, forbidden={5, 77, 4242})
    a = np.frombuffer(z, dtype=np.uint8).astype(np.int64)
    code = (a[:-2] << 16) | (a[1:-1] << 8) | a[2:]
    assert len(np.unique(code)) == len(code) and not np.isin(P.buckets_at(z), [5, 77, 4242]).any()
    assert P.bucket(b"abc") == ((97 << 10) ^ (98 << 5) ^ 99) & 0x7FFF
    pr = bytes([200, 220, 240, 201])
    for fl in ("tri", "bkt"):
        d = P.decoy(pr, 5, fl)
        assert P.bucket(d[:3]) == P.bucket(pr[:3]) and (d[:3] == pr[:3]) == (fl == "tri") and d[3] != pr[3]


@pytest.mark.skipif(not R.available(), reason="compiled reference not built (oracle/_ref/libzref.so)")
def test_reference_gives_the_golden_bytes(cat, gold):
    from oracle import gen_golden_parse as G
    bad = [c.name for c in cat if G.rows_of(c) != gold[c.name]]
    assert not bad, (len(bad), bad[:8])
