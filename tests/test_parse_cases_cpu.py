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
            _, t = O.deflate_cont_tokens(c.data, k.level, k.strategy)
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
                z = O.deflate_cont(c.data, P.CONFIGS[cfg].level)
                got = [len(z), h16(z)]
            else:
                zs = [chunk(c, cfg, last) for last in (0, 1)]
                got = [[len(z), h16(z)] for z in zs]
            if got != want:
                bad.append((c.name, cfg, got, want))
            if cfg in gold[c.name].get("cont", {}):
                z = O.deflate_cont(c.data, P.CONFIGS[cfg].level)
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
    assert ncont >= 9 * 12 * 2


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
    assert fam == {"chain", "quarter", "nice", "clip", "tie", "stairs", "lazy", "short", "reach", "fast", "placed"}
    names = {c.name for c in cat}
    for cfg in P.FAST + P.SLOW:
        chain = P.row(cfg)[3]
        for d in (chain - 1, chain, chain + 1):
            assert {"chain-%s-%s-d%d" % (cfg, fl, d) for fl in ("tri", "bkt")} <= names
    assert P.row("T13")[3] >> 2 == 3 and P.row("T100")[3] >> 2 == 25 and P.row("T33")[3] == 33
    assert not any(c.family == "quarter" and c.cfgs == ["L4"] for c in cat)  # (good_length == max_lazy: unreachable, see parsecases)
    assert all(len(c.data) <= 65536 for c in cat if not c.cont)
    assert max(len(c.data) for c in cat if c.family == "chain" and c.cfgs == ["L9"]) < 26000
    edges = {p for c in cat if c.cont for p, _ in c.claims[c.cfgs[0]]}
    assert edges == {65023, 65024, 65025, 97535, 97536, 97537}


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
