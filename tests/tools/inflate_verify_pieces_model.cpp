// The verify form of the piece path (zlib_amd/csrc/zgpu_inflate_pieces_plan.h, and pieces_verify_confirm of zgpu_common.h), printed on a machine without a
// GPU: built for the host only, so pieces_select, pieces_verify_chain and pieces_verify_confirm below are the very functions the device runs.  One command per run:
//   geom MIN BODY...                          body=.. long=.. ntargets=.. cap=.. per body
//   select SPACING FIRST_BIT END CAP DYN STO INPUT          starts=..   DYN, STO: comma lists, one entry per finder, - for none
//   verdict BODY_LO IN_HI STARTS ENDS CHECKS DO INPUT       chain=.. used=.. total=.. end_bit=.. ostart=.. clean=.. adler=.. crc=..
//         STARTS: comma list of bits, a stored start with the suffix s; ENDS: comma list of END_BIT:OUT_BYTES:FLAGS (FLAGS - : never written);
//         CHECKS: comma list of END_BIT:OUT_BYTES:FLAGS:ADLER32:CRC32, one per piece (FLAGS - : never written); DO: bit 0 Adler-32, bit 1 CRC-32
//   join DO OUT_BYTES:ADLER32:CRC32...        clean=.. adler=.. crc=..   the pieces' own values (each from 1 and 0) joined in order
//   plan NITEMS NTARGETS NPIECES              total=.. per=.. and name=off:bytes per region
//   rounds SLOT_KNOB NTARGETS:CAP...          first=.. last=.. slots=.. targets=.. plan=.. cap=.. per round (SLOT_KNOB 0: the default cap)
// INPUT: the buffer the starts lie in -- @FILE (its bytes), or a comma list of POS:BYTE over zeros, or - for zeros; IN_HI / END + 16 bytes at least
#include "../../zlib_amd/csrc/zgpu_common.h"
#include "../../zlib_amd/csrc/zgpu_inflate_pieces_plan.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace zgpu;

struct Row { uint64_t start; };

static std::vector<std::string> split(const std::string &s, char sep)
{
    std::vector<std::string> out;
    if (s == "-") return out;
    size_t at = 0;
    for (;;) {
        const size_t e = s.find(sep, at);
        out.push_back(s.substr(at, e == std::string::npos ? e : e - at));
        if (e == std::string::npos) break;
        at = e + 1;
    }
    return out;
}
static uint64_t num(const std::string &s) { return s == "-" ? kPiecesNone : strtoull(s.c_str(), nullptr, 10); }

static bool input(const std::string &arg, uint64_t least, std::vector<uint8_t> *in)
{
    in->assign(least + 16, 0);
    if (arg == "-") return true;
    if (arg[0] == '@') {
        FILE *f = fopen(arg.c_str() + 1, "rb");
        if (!f) return false;
        std::vector<uint8_t> got;
        uint8_t buf[65536];
        for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) got.insert(got.end(), buf, buf + n);
        fclose(f);
        if (got.size() > in->size()) in->resize(got.size() + 16, 0);
        memcpy(in->data(), got.data(), got.size());
        return true;
    }
    for (const std::string &s : split(arg, ',')) {
        const std::vector<std::string> f = split(s, ':');
        if (f.size() != 2 || num(f[0]) >= in->size()) return false;
        (*in)[num(f[0])] = (uint8_t)num(f[1]);
    }
    return true;
}

static PieceCheck check_of(uint64_t end_bit, uint32_t out_bytes, uint32_t flags, uint32_t adler, uint32_t crc)
{
    PieceCheck c{};
    c.end_bit = end_bit; c.out_bytes = out_bytes; c.flags = flags; c.adler_a = adler & 0xFFFFu; c.adler_b = adler >> 16; c.crc = crc;
    return c;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "geom" && argc >= 3) {
        const uint64_t min_bytes = num(argv[2]);
        for (int i = 3; i < argc; i++) {
            const uint64_t body = num(argv[i]);
            const PiecesGeom g = pieces_geom(body);
            printf("body=%" PRIu64 " long=%d ntargets=%u cap=%u\n", body, pieces_long(body, min_bytes) ? 1 : 0, g.ntargets, g.piece_cap);
        }
        return 0;
    }
    if (cmd == "select" && argc == 9) {
        const uint64_t spacing = num(argv[2]), first_bit = num(argv[3]), end = num(argv[4]);
        const uint32_t cap = (uint32_t)num(argv[5]);
        std::vector<uint64_t> dyn, sto;
        for (const std::string &s : split(argv[6], ',')) dyn.push_back(num(s));
        for (const std::string &s : split(argv[7], ',')) sto.push_back(num(s));
        std::vector<uint8_t> in;
        if (dyn.size() != sto.size() || !input(argv[8], end, &in)) return 2;
        std::vector<uint64_t> starts(cap + 1, 0);
        const uint32_t n = pieces_select(dyn.data(), sto.data(), (uint32_t)dyn.size(), in.data(), first_bit, end, spacing, starts.data(), cap);
        printf("starts=");
        for (uint32_t i = 0; i < n; i++) printf("%s%" PRIu64 "%s", i ? "," : "", starts[i] & ~kPiecesStoredFlag, (starts[i] & kPiecesStoredFlag) ? "s" : "");
        printf("\n");
        return 0;
    }
    if (cmd == "verdict" && argc == 9) {
        const uint64_t body_lo = num(argv[2]), in_hi = num(argv[3]);
        const uint32_t want = (uint32_t)num(argv[7]);
        std::vector<Row> rows;
        std::vector<SpecEnd> ends;
        std::vector<PieceCheck> checks;
        for (const std::string &s : split(argv[4], ',')) {
            const bool st = !s.empty() && s.back() == 's';
            rows.push_back(Row{num(st ? s.substr(0, s.size() - 1) : s) | (st ? kPiecesStoredFlag : 0)});
        }
        for (const std::string &s : split(argv[5], ',')) {
            const std::vector<std::string> f = split(s, ':');
            if (f.size() != 3) return 2;
            ends.push_back(f[2] == "-" ? SpecEnd{~0ull, ~0u, ~0u} : SpecEnd{num(f[0]), (uint32_t)num(f[1]), (uint32_t)num(f[2])});
        }
        for (const std::string &s : split(argv[6], ',')) {
            const std::vector<std::string> f = split(s, ':');
            if (f.size() != 5) return 2;
            checks.push_back(f[2] == "-" ? check_of(~0ull, ~0u, ~0u, ~0u, ~0u) : check_of(num(f[0]), (uint32_t)num(f[1]), (uint32_t)num(f[2]), (uint32_t)num(f[3]), (uint32_t)num(f[4])));
        }
        std::vector<uint8_t> in;
        if (rows.size() != ends.size() || rows.size() != checks.size() || !input(argv[8], in_hi, &in)) return 2;
        std::vector<uint64_t> ostart(rows.size() + 1, 0);
        const PiecesSizesVerdict v = pieces_verify_chain(ends.data(), rows.data(), (uint32_t)rows.size(), in.data(), body_lo, in_hi, ostart.data());
        PiecesJoined j{1, 0, 0};
        const bool clean = v.clean && pieces_verify_confirm(ends.data(), checks.data(), v.used, want & 1u, (want >> 1) & 1u, &j);
        printf("chain=%u used=%u total=%" PRIu64 " end_bit=%" PRIu64 " ostart=", v.clean, v.used, v.total, v.end_bit);
        for (uint32_t i = 0; i < v.used; i++) printf("%s%" PRIu64, i ? "," : "", ostart[i]);
        printf("%s clean=%d adler=%u crc=%u\n", v.used ? "" : "-", clean ? 1 : 0, j.a | (j.b << 16), j.crc);
        return 0;
    }
    if (cmd == "join" && argc >= 3) {
        const uint32_t want = (uint32_t)num(argv[2]);
        std::vector<SpecEnd> ends;
        std::vector<PieceCheck> checks;
        for (int i = 3; i < argc; i++) {
            const std::vector<std::string> f = split(argv[i], ':');
            if (f.size() != 3) return 2;
            ends.push_back(SpecEnd{(uint64_t)i, (uint32_t)num(f[0]), i + 1 == argc ? 1u : 0u});
            checks.push_back(check_of((uint64_t)i, (uint32_t)num(f[0]), i + 1 == argc ? 1u : 0u, (uint32_t)num(f[1]), (uint32_t)num(f[2])));
        }
        PiecesJoined j{1, 0, 0};
        const bool clean = pieces_verify_confirm(ends.data(), checks.data(), (uint32_t)ends.size(), want & 1u, (want >> 1) & 1u, &j);
        printf("clean=%d adler=%u crc=%u\n", clean ? 1 : 0, j.a | (j.b << 16), j.crc);
        return 0;
    }
    if (cmd == "plan" && argc == 5) {
        const PiecesVerifyRoundPlan p = pieces_verify_round_plan(num(argv[2]), num(argv[3]), num(argv[4]));
        printf("total=%" PRIu64 " per=%" PRIu64, p.total, kPiecesVerifyPerPieceBytes);
        for (int i = 0; i < kPiecesVerifyRegions; i++) printf(" %s=%" PRIu64 ":%" PRIu64, pieces_verify_region_name(i), pieces_verify_region(p, i).off, pieces_verify_region(p, i).bytes);
        printf("\n");
        return 0;
    }
    if (cmd == "rounds" && argc >= 3) {
        const uint64_t slot_cap = pieces_verify_slot_cap(num(argv[2]));
        std::vector<PiecesItemCost> c;
        for (int i = 3; i < argc; i++) {
            const std::vector<std::string> f = split(argv[i], ':');
            if (f.size() != 2) return 2;
            c.push_back(PiecesItemCost{0, (uint32_t)num(f[0]), (uint32_t)num(f[1])});
        }
        for (uint64_t first = 0; first < c.size();) {
            const uint64_t last = pieces_sizes_round_end(c.data(), c.size(), first, slot_cap);
            if (last <= first) return 3; // (a round that takes nothing would never end)
            uint64_t slots = 0, targets = 0;
            for (uint64_t k = first; k < last; k++) { slots += c[k].piece_cap; targets += c[k].ntargets; }
            printf("first=%" PRIu64 " last=%" PRIu64 " slots=%" PRIu64 " targets=%" PRIu64 " plan=%" PRIu64 " cap=%" PRIu64 "\n", first, last, slots, targets,
                   pieces_verify_round_plan(last - first, targets, slots).total, slot_cap);
            first = last;
        }
        return 0;
    }
    return 2;
}
