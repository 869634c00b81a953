"""The round catalogue (oracle/roundcases.py) is what it says it is -- no GPU.  The restatement gives the golden bytes (tests/golden/round_kat.json, the
compiled reference's, oracle/gen_golden_rounds.py), every claim holds in its tokens, the two sides of a pair differ, the probes have the candidates they
were built with, and -- what makes a case a test of the rounds at all -- the WARM-UP of the probe's tile, a parse of the stream's suffix from the tile's
history on, gets the probe's candidate wrong exactly as the case says: a case whose guess is right tests nothing and fails here."""
import hashlib

import numpy as np
import pytest

from oracle import blockwalk as BW, oracle_py as O, parsecases as P, refzlib as R, roundcases as RC


def h16(b):
    return hashlib.sha256(b).hexdigest()[:16]


@pytest.fixture(scope="module")
def cat():
    return RC.catalogue()


@pytest.fixture(scope="module")
def gold(golden):
    return golden("round_kat.json")["cases"]


_parses = {}


def tokens(data, level):
    return O.deflate_cont_tokens(data, level)[1]


def accounts(c, cfg, tile=None):
    """(stream's parse, warm-up's parse, stream's chains, warm-up's chains) of the case's tile, computed once"""
    key = (c.name, cfg, tile or c.tile)
    if key not in _parses:
        _parses[key] = RC.warm_account(c.data, tile or c.tile, RC.level_of(cfg), tokens)
    return _parses[key]


def test_catalogue_is_the_one_the_golden_file_names(cat, gold):
    names = [c.name for c in cat]
    assert len(set(names)) == len(names) and set(names) == set(gold)
    again = RC.build_catalogue()
    assert [(c.name, h16(c.data), c.claims, c.guess) for c in again] == [(c.name, h16(c.data), c.claims, c.guess) for c in cat]
    for c in cat:
        assert gold[c.name]["data"] == [len(c.data), h16(c.data)], c.name
        assert RC.ntiles(len(c.data)) <= 8 and set(c.cfgs) == set(P.FAST), c.name
        for cfg in c.cfgs:
            assert gold[c.name]["claims"][cfg] == [[p, 0, 1] if t == P.LIT else [p, t[0], t[1]] for p, t in c.claims[cfg]], (c.name, cfg)


def test_families_the_catalogue_must_hold(cat):
    fam = {}
    for c in cat:
        fam.setdefault(c.family, []).append(c)
    assert set(fam) == {"guess", "reach", "entry", "chain"}
    g = fam["guess"]
    # both polarities, at 32505 / 32506 / 32507, inside and outside the long match; the first own position of the tile; tiles 2 and 3
    assert {(c.guess["stream"], c.guess["warm"]) for c in g} == {(0, 1), (1, 0), (1, 1)}
    for pol in ((0, 1), (1, 0)):
        assert {c.probe - c.guess["q"] for c in g if (c.guess["stream"], c.guess["warm"]) == pol} == {P.MAX_DIST - 1, P.MAX_DIST, P.MAX_DIST + 1}
    assert any(c.probe == RC.own(c.tile) for c in g) and {c.tile for c in g} == {1, 2, 3}
    # reach: three tiles, k + 32506 at window offsets 0, 1, 63 and in the tile's last window, each with its partner at k + 32507
    r = fam["reach"]
    assert all(c.tile == 2 and RC.ntiles(len(c.data)) >= 3 and c.guess["k"] == c.guess["q"] >= RC.hist(2) + 6 for c in r)
    on = [c for c in r if c.probe - c.guess["k"] == P.MAX_DIST]
    assert {c.probe % 64 for c in on} >= {0, 1, 63} and any(c.probe >= RC.own(2) + RC.TILE - 64 for c in on)
    assert sorted(c.guess["k"] for c in on) == sorted(c.guess["k"] for c in r if c.probe - c.guess["k"] == P.MAX_DIST + 1)
    assert sorted(abs(c.guess["exits"][1] - c.guess["exits"][0]) for c in fam["entry"] if "exits" in c.guess) == [1, 2, 257]  # how far the predecessor's exit moves
    back = [c.guess["exits3"] for c in fam["entry"] if "exits3" in c.guess]
    assert back and all(a == z != m for a, m, z in back) and all(RC.ntiles(len(c.data)) >= 4 for c in fam["entry"] if "exits3" in c.guess)  # an exit that moves and moves back
    assert all(c.guess["travel"] >= 4 and len(c.guess["probes"]) == c.guess["travel"] for c in fam["chain"])
    feeds = RC.feed_cases()
    assert {c.family for c in feeds} == {"guess", "reach"} and all([r[1][0][0] for r in RC.feed_rows(c)][:5] == [RC.own(c.tile) - g_ for g_ in (0, 1, 31, 32, 33)] for c in feeds)


def test_restatement_gives_the_golden_bytes(cat, gold):
    bad = []
    for c in cat:
        for cfg in c.cfgs:
            z = O.cont_stream(c.data, RC.level_of(cfg), (), wbits=-15)
            if [len(z), h16(z)] != gold[c.name]["out"][cfg]:
                bad.append((c.name, cfg, len(z)))
        for tag, calls, _ in (RC.feed_rows(c) if "feed" in gold[c.name] else []):
            for cfg in c.cfgs:
                z = O.cont_stream(c.data, RC.level_of(cfg), calls, wbits=-15)
                if [len(z), h16(z)] != gold[c.name]["feed"][tag][cfg]:
                    bad.append((c.name, tag, cfg, len(z)))
    assert not bad, bad[:12]


def test_every_claim_holds(cat):
    bad = []
    for c in cat:
        for cfg in c.cfgs:
            s = accounts(c, cfg)[0]
            assert c.claims[cfg], c.name
            bad += [(c.name, cfg, p, want, RC.token_at(*s, p)) for p, want in c.claims[cfg] if RC.token_at(*s, p) != want]
    assert not bad, bad[:12]


def test_full_flush_forgets_the_candidate(cat):
    """behind a Z_FULL_FLUSH at the tile's first position the probe is a literal, whatever the chains held (the sync flush keeps them: its row has the plain claim)"""
    for c in RC.feed_cases():
        tag, calls, claims = RC.feed_rows(c)[-1]
        assert tag == "full" and calls[0][1] == RC.Z_FULL_FLUSH
        cut = calls[0][0]
        assert cut <= c.probe
        for cfg in c.cfgs:  # (behind a full flush the parse is a parse from nothing)
            s = RC.starts_of(tokens(c.data[cut:], RC.level_of(cfg)))
            for p, want in claims:
                assert RC.token_at(*s, p - cut) == want, (c.name, cfg, p)


def test_pairs_differ(cat):
    groups = {}
    for c in cat:
        if c.pair:
            groups.setdefault(c.pair[0], {})[c.pair[1]] = c
    assert len(groups) >= 10
    for g, sides in groups.items():
        assert set(sides) == {0, 1}, g
        for cfg in P.FAST:
            # (the token at the probe and the one a literal there would be followed by: with the candidate out of the chains the reference takes the NEXT one)
            a, b = ([RC.token_at(*accounts(sides[k], cfg)[0], sides[k].probe + i) for i in (0, 1)] for k in (0, 1))
            assert a[0] is not None and b[0] is not None and a != b, (g, cfg, a, b)


def test_candidate_counts_are_as_built(cat):
    for c in cat:
        assert P.chain_of(c.data, c.probe) == c.chain, c.name
        assert len(c.chain) == (1 if c.probe - c.guess["q"] <= P.MAX_DIST else 0), c.name
        for tile, t, cand in c.guess.get("probes", []):
            assert P.chain_of(c.data, t) == [cand] and t - cand == P.MAX_DIST and RC.own(tile) <= t < RC.own(tile) + RC.TILE, (c.name, tile)


def test_the_guess_is_wrong_where_the_case_says(cat):
    seen = 0
    for c in cat:
        g = c.guess
        for cfg in c.cfgs:
            s, w, si, wi = accounts(c, cfg)
            q = g["q"]
            assert RC.hist(c.tile) + 6 <= q < RC.own(c.tile), c.name
            assert (int(si[q]), int(wi[q])) == (g["stream"], g["warm"]), (c.name, cfg, "the candidate's bit")
            k = RC.highest_difference(si, wi, c.tile)
            assert k == g["k"] and bool(si[k]) != bool(wi[k]) and np.array_equal(si[k + 1: RC.own(c.tile)], wi[k + 1: RC.own(c.tile)]), (c.name, cfg, k)
            assert RC.token_at(*w, c.probe) == g["token"], (c.name, cfg, "what the warm-up starts at the probe")
            wrong = RC.token_at(*w, c.probe) != RC.token_at(*s, c.probe)
            assert wrong == (g["stream"] != g["warm"] and c.probe - q <= P.MAX_DIST), (c.name, cfg)
            seen += wrong
            if "exits" in g:  # the predecessor of the tile that is entered anew: its exit by the guess, by the stream
                edge = RC.own(c.tile) + RC.TILE
                assert (RC.exit_at(w[0], w[1], edge), RC.exit_at(s[0], s[1], edge)) == g["exits"] and g["exits"][0] != g["exits"][1], (c.name, cfg)
            if "exits3" in g:  # tile exit_tile's exit round by round: by its own warm-up (round 0), parsed behind the GUESS of the tile in front (round 1: the suffix
                # parse from that tile's history on goes on into this tile from that tile's guessed exit with its guessed bits), by the stream (round 2)
                x = g["exit_tile"]
                edge = RC.own(x) + RC.TILE
                own_warm = accounts(c, cfg, x)[1]
                assert c.tile == x - 1 and (RC.exit_at(own_warm[0], own_warm[1], edge), RC.exit_at(w[0], w[1], edge), RC.exit_at(s[0], s[1], edge)) == g["exits3"], (c.name, cfg)
                t2, src = g["run"]   # the run's first token: the warm-up of its own tile and the stream take it, the parse behind the guess cannot (its candidate is inside a match there)
                assert RC.token_at(*own_warm, t2) == RC.token_at(*s, t2) == (t2 - src, P.MAXM) and RC.token_at(*w, t2) == P.LIT and bool(si[src]) and not wi[src], (c.name, cfg)
            for tile, t, cand in g.get("probes", []):  # every tile's warm-up takes its probe's candidate; the reference takes it in every other tile
                sw = accounts(c, cfg, tile)
                assert RC.token_at(*sw[1], t) == g["token"] and bool(sw[3][cand]), (c.name, cfg, tile)
                assert (RC.token_at(*s, t) == g["token"]) == (tile % 2 == 0), (c.name, cfg, tile)
    assert seen >= 3 * 12


def test_readable_failure_names_the_token():
    """what tests/test_gpu_round_cases.py reports on a mismatch (oracle/blockwalk.py first_token_difference): a valid stream against its own tokens, and against
    tokens that have at the probe what the warm-up would have made of it"""
    c = next(c for c in RC.catalogue() if c.family == "guess" and c.guess["stream"] != c.guess["warm"] and c.probe - c.guess["q"] == P.MAX_DIST)
    z, toks = O.deflate_cont_tokens(c.data, 1)
    st, ln, dist = RC.starts_of(toks)
    want = list(zip(st.tolist(), dist.tolist(), ln.tolist()))
    assert BW.first_token_difference(z, want).startswith("the first %d tokens agree, 0 follow" % len(want))
    i = st.tolist().index(c.probe)
    wrong = want[:i] + [(c.probe, P.MAX_DIST, 20)] + want[i + 1:]  # (what the warm-up would have made of the probe)
    msg = BW.first_token_difference(z, wrong)
    assert msg.startswith("token %d at position %d: (dist 0, len 1), the reference has (dist %d, len 20)" % (i, c.probe, P.MAX_DIST)), msg


@pytest.mark.skipif(not R.available(), reason="compiled reference not built (oracle/_ref/libzref.so)")
def test_reference_gives_the_golden_bytes(cat, gold):
    for c in cat[::5]:
        for cfg in c.cfgs:
            z = R.deflate_calls(c.data, RC.level_of(cfg), (), wbits=-15)
            assert [len(z), h16(z)] == gold[c.name]["out"][cfg], (c.name, cfg)


def test_an_exit_is_its_last_tokens_end(cat):
    """What stands for the case the catalogue leaves out ("only the exit differs while every token the tile made is the same"): a tile's exit is where the last token
    that starts in it ends, so two parses of a tile that enter at the same position and make the same tokens leave at the same position -- recomputed here from
    the tokens of the stream and of the warm-up for the probe's tile of every case, with the converse on the cases whose exits differ."""
    for c in cat:
        edge = RC.own(c.tile) + RC.TILE
        if edge > len(c.data):
            continue
        for cfg in c.cfgs:
            s, w = accounts(c, cfg)[:2]
            res = []
            for st, ln, _ in (s, w):
                i = int(np.searchsorted(st, RC.own(c.tile)))        # the first token that starts in the tile, (its start - the tile's) being the entry
                j = int(np.searchsorted(st, edge))                  # ... and the first that does not
                inside = list(zip(st[i:j].tolist(), ln[i:j].tolist()))
                assert RC.exit_at(st, ln, edge) == inside[-1][0] + inside[-1][1] - edge, (c.name, cfg)
                res.append((inside, RC.exit_at(st, ln, edge)))
            assert (res[0][0] != res[1][0]) or res[0][1] == res[1][1], (c.name, cfg)
            if "exits" in c.guess:
                assert res[0][1] != res[1][1] and res[0][0] != res[1][0], (c.name, cfg)
