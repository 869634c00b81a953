// The sizing form of the piece path (zlib_amd/csrc/zgpu_inflate_pieces_plan.h), printed on a machine without a GPU: the header is host code here
// (ZGPU_PIECES_HD is empty), so pieces_select and pieces_sizes_chain below are the very functions the device runs.  One command per run:
//   geom MIN BODY...                          body=.. long=.. ntargets=.. cap=.. per body
//   select SPACING FIRST_BIT END CAP DYN STO INPUT          starts=..   DYN, STO: comma lists, one entry per finder, - for none
//   chain BODY_LO IN_HI STARTS ENDS NEEDS INPUT             total=.. end_bit=.. used=.. clean=..
//         STARTS: comma list of bits, a stored start with the suffix s; ENDS: comma list of END_BIT:OUT_BYTES:FLAGS (FLAGS - : never written);
//         NEEDS: comma list, one per piece
//   plan NITEMS NTARGETS NPIECES              total=.. and name=off:bytes per region
//   rounds SLOT_CAP NTARGETS:CAP...           first=.. last=.. slots=.. targets=.. scratch=.. per round
// INPUT: the buffer the starts lie in -- @FILE (its bytes), or a comma list of POS:BYTE over zeros, or - for zeros; IN_HI / END + 16 bytes at least
#include "../../zlib_amd/csrc/zgpu_inflate_pieces_plan.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace zgpu;

struct End { uint64_t end_bit; uint32_t out_bytes, flags; };
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
    if (cmd == "chain" && argc == 8) {
        const uint64_t body_lo = num(argv[2]), in_hi = num(argv[3]);
        std::vector<Row> rows;
        std::vector<End> ends;
        std::vector<uint32_t> need;
        for (const std::string &s : split(argv[4], ',')) {
            const bool st = !s.empty() && s.back() == 's';
            rows.push_back(Row{num(st ? s.substr(0, s.size() - 1) : s) | (st ? kPiecesStoredFlag : 0)});
        }
        for (const std::string &s : split(argv[5], ',')) {
            const std::vector<std::string> f = split(s, ':');
            if (f.size() != 3) return 2;
            ends.push_back(f[2] == "-" ? End{~0ull, ~0u, ~0u} : End{num(f[0]), (uint32_t)num(f[1]), (uint32_t)num(f[2])});
        }
        for (const std::string &s : split(argv[6], ',')) need.push_back((uint32_t)num(s));
        std::vector<uint8_t> in;
        if (rows.size() != ends.size() || rows.size() != need.size() || !input(argv[7], in_hi, &in)) return 2;
        const PiecesSizesVerdict v = pieces_sizes_chain(ends.data(), need.data(), rows.data(), (uint32_t)rows.size(), in.data(), body_lo, in_hi);
        printf("total=%" PRIu64 " end_bit=%" PRIu64 " used=%u clean=%u\n", v.total, v.end_bit, v.used, v.clean);
        return 0;
    }
    if (cmd == "plan" && argc == 5) {
        const PiecesSizesRoundPlan p = pieces_sizes_round_plan(num(argv[2]), num(argv[3]), num(argv[4]));
        printf("total=%" PRIu64, p.total);
        for (int i = 0; i < kPiecesSizesRegions; i++) printf(" %s=%" PRIu64 ":%" PRIu64, pieces_sizes_region_name(i), pieces_sizes_region(p, i).off, pieces_sizes_region(p, i).bytes);
        printf("\n");
        return 0;
    }
    if (cmd == "rounds" && argc >= 3) {
        const uint64_t slot_cap = num(argv[2]);
        std::vector<PiecesItemCost> c;
        for (int i = 3; i < argc; i++) {
            const std::vector<std::string> f = split(argv[i], ':');
            if (f.size() != 2) return 2;
            c.push_back(PiecesItemCost{0, (uint32_t)num(f[0]), (uint32_t)num(f[1])});
        }
        for (uint64_t first = 0; first < c.size();) {
            const uint64_t last = pieces_sizes_round_end(c.data(), c.size(), first, slot_cap);
            if (last <= first) return 3; // (a round that takes nothing would never end)
            uint64_t slots = 0, targets = 0, scratch = 0;
            for (uint64_t k = first; k < last; k++) { slots += c[k].piece_cap; targets += c[k].ntargets; scratch += pieces_sizes_item_scratch(c[k]); }
            printf("first=%" PRIu64 " last=%" PRIu64 " slots=%" PRIu64 " targets=%" PRIu64 " scratch=%" PRIu64 "\n", first, last, slots, targets, scratch);
            first = last;
        }
        return 0;
    }
    return 2;
}
