// What zlib_amd/csrc/zgpu_inflate_pieces_plan.h decides, printed on a machine without a GPU: the header is host code here (ZGPU_PIECES_HD is empty), so
// pieces_select below is the very function pieces_select_kernel runs on the device.  One command per run:
//   geom MIN BODY...                          body=.. long=.. spacing=.. fspacing=.. ntargets=.. cap=.. per body
//   plan NITEMS NTARGETS NPIECES ROOM         total=.. page_cap=.. and name=off:bytes per region
//   rounds ROUND_BYTES ROOM:NTARGETS:CAP...   first=.. last=.. room=.. scratch=.. per round
//   select SPACING FIRST_BIT END CAP DYN STO LENS   starts=..   DYN, STO: comma lists, one entry per finder, - for none; LENS: comma list of POS:LEN, the
//                                             16-bit LEN stored at byte POS of the (otherwise zero) input of END bytes; - for none
#include "../../zlib_amd/csrc/zgpu_inflate_pieces_plan.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace zgpu;

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

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    if (cmd == "geom" && argc >= 3) {
        const uint64_t min_bytes = num(argv[2]);
        for (int i = 3; i < argc; i++) {
            const uint64_t body = num(argv[i]);
            const PiecesGeom g = pieces_geom(body);
            printf("body=%" PRIu64 " long=%d spacing=%" PRIu64 " fspacing=%" PRIu64 " ntargets=%u cap=%u\n", body, pieces_long(body, min_bytes) ? 1 : 0, g.spacing, g.fspacing, g.ntargets,
                   g.piece_cap);
        }
        return 0;
    }
    if (cmd == "plan" && argc == 6) {
        const PiecesRoundPlan p = pieces_round_plan(num(argv[2]), num(argv[3]), num(argv[4]), num(argv[5]));
        printf("total=%" PRIu64 " page_cap=%" PRIu64, p.total, p.page_cap);
        for (int i = 0; i < kPiecesRegions; i++) printf(" %s=%" PRIu64 ":%" PRIu64, pieces_region_name(i), pieces_region(p, i).off, pieces_region(p, i).bytes);
        printf("\n");
        return 0;
    }
    if (cmd == "rounds" && argc >= 3) {
        const uint64_t round_bytes = num(argv[2]);
        std::vector<PiecesItemCost> c;
        for (int i = 3; i < argc; i++) {
            const std::vector<std::string> f = split(argv[i], ':');
            if (f.size() != 3) return 2;
            c.push_back(PiecesItemCost{num(f[0]), (uint32_t)num(f[1]), (uint32_t)num(f[2])});
        }
        for (uint64_t first = 0; first < c.size();) {
            const uint64_t last = pieces_round_end(c.data(), c.size(), first, round_bytes);
            if (last <= first) return 3; // (a round that takes nothing would never end)
            uint64_t room = 0, scratch = 0;
            for (uint64_t k = first; k < last; k++) { room += c[k].room; scratch += pieces_item_scratch(c[k]); }
            printf("first=%" PRIu64 " last=%" PRIu64 " room=%" PRIu64 " scratch=%" PRIu64 "\n", first, last, room, scratch);
            first = last;
        }
        return 0;
    }
    if (cmd == "select" && argc == 9) {
        const uint64_t spacing = num(argv[2]), first_bit = num(argv[3]), end = num(argv[4]);
        const uint32_t cap = (uint32_t)num(argv[5]);
        std::vector<uint64_t> dyn, sto;
        for (const std::string &s : split(argv[6], ',')) dyn.push_back(num(s));
        for (const std::string &s : split(argv[7], ',')) sto.push_back(num(s));
        if (dyn.size() != sto.size()) return 2;
        std::vector<uint8_t> in(end + 1, 0);
        for (const std::string &s : split(argv[8], ',')) {
            const std::vector<std::string> f = split(s, ':');
            if (f.size() != 2 || num(f[0]) + 2 > end) return 2;
            in[num(f[0])] = (uint8_t)(num(f[1]) & 255u); in[num(f[0]) + 1] = (uint8_t)(num(f[1]) >> 8);
        }
        std::vector<uint64_t> starts(cap + 1, 0);
        const uint32_t n = pieces_select(dyn.data(), sto.data(), (uint32_t)dyn.size(), in.data(), first_bit, end, spacing, starts.data(), cap);
        printf("starts=");
        for (uint32_t i = 0; i < n; i++) printf("%s%" PRIu64 "%s", i ? "," : "", starts[i] & ~kPiecesStoredFlag, (starts[i] & kPiecesStoredFlag) ? "s" : "");
        printf("\n");
        return 0;
    }
    return 2;
}
