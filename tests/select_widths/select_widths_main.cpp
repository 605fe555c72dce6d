// select_widths_main.cpp -- TEST-ONLY stand-alone program: Flow::select() of the stage-parallel kernel
// (asyncflow_amd/csrc/af_flow.hpp) with a lane window of its own width per station list (AF_SELECT_WINDOW_S0 .. _S3), on crafted
// station lists, on the 64-fibre wave emulator of tests/hostcheck.
//
// Built by tests/test_flow_select_widths.py with the default widths, with every list at width 1, 2 and 4, with four different
// widths, without the window, and once under AddressSanitizer + UBSan.  The lists do not depend on the build: every case is held
// to a scalar restatement of the selection (a stable sort of the eligible keys) and to the path it must take at the width of ITS
// list (the proof restated on the keys, against aff::g_select_window_by_list), and asserts that the window's ranked calls with
// entries kept, with fewer selected than eligible, and the calls the window did not rank each occurred; the program prints one line per case with every
// output word, and the test holds the lines of all builds to each other.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../asyncflow_amd/csrc/af_plan_pack.hpp"
#include "../../asyncflow_amd/csrc/af_flow_host.hpp"
#include "../hostcheck/wave_emul.hpp"

namespace {

constexpr double kLo = 1.0, kHi = 2.0, kBeyond = 2.5;   // horizon of the station, bound of the call, a key that is not eligible
constexpr uint32_t kWidest = 8u;                        // no build of the test has a wider window: an inversion further apart fails every proof

struct Case {
    const char* name;
    std::vector<double> key;
    uint32_t room;
};

struct Result {
    uint32_t n_sel = 0, kept = 0, why = 0;
    double H = 0.0;
    double okey[64], ot0[64];
    uint32_t oaux[64];
    std::vector<double> lkey, lt0;
    std::vector<uint32_t> laux;
};

uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
}
double t0_of(uint32_t i) { return 0.25 + 0.001 * i; }
uint32_t aux_of(uint32_t i) { return (i * 0x9E37u + 0x8001u) & 0xFFFFu; }   // all sixteen bits of the aux word in use

template <uint32_t FEAT>
Result run_select(const Case& c, uint32_t s) {
    using F = aff::Flow<emu::WaveEmu, 1u, FEAT>;
    aff::FlowArgs A{};
    A.total_time = 10.0;
    A.n_edges = 6u;
    A.n_servers = 2u;
    A.L = aff::make_flow_layout(64u, 64u, 8u, 1u, A.n_edges, A.n_servers, 0u);
    std::vector<uint64_t> lds(A.L.n_words, 0xFFF8DEADBEEF0000ull);   // (stale words read as NaN keys)
    const uint32_t n = (uint32_t)c.key.size();
    const bool has_aux = s == 2u || ((FEAT & aff::FEAT_FAR) != 0u && s == 3u);
    {
        F f(A);
        f.M = lds.data();
        for (uint32_t i = 0; i < n; ++i) {
            f.list_key(s)[i] = c.key[i];
            f.list_t0(s)[i] = t0_of(i);
            if (has_aux) f.list_aux(s)[i] = (uint16_t)aux_of(i);
        }
    }
    Result r;
    uint32_t why_of[64];
    emu::run_wave([&]() {
        F f(A);
        f.M = lds.data();
        f.blob = nullptr;
        f.lane = emu::WaveEmu::lane();
        f.nl0 = f.nl1 = f.nl2 = f.nl3 = 0u;
        f.h0 = f.h1 = f.h2 = f.h3 = kLo;
        f.t_lim = 1e300;
        f.moved = false;
        f.why = 0u;
        f.n_list_set(s, n);
        double okey, ot0;
        uint32_t oaux;
        const uint32_t n_sel = f.select(s, kHi, c.room, okey, ot0, oaux, s);
        r.okey[f.lane] = okey;
        r.ot0[f.lane] = ot0;
        r.oaux[f.lane] = oaux;
        why_of[f.lane] = f.why;
        if (f.lane == 0u) {
            r.n_sel = n_sel;
            r.kept = f.n_list_get(s);
            r.H = f.H_get(s);
        }
    });
    for (uint32_t l = 0; l < 64u; ++l) r.why |= why_of[l];
    F f(A);
    f.M = lds.data();
    for (uint32_t i = 0; i < r.kept; ++i) {
        r.lkey.push_back(f.list_key(s)[i]);
        r.lt0.push_back(f.list_t0(s)[i]);
        r.laux.push_back(has_aux ? f.list_aux(s)[i] : 0u);
    }
    return r;
}

int g_failed = 0;
int g_ranked_kept = 0, g_ranked_short = 0;   // cases that must be ranked by the window with entries kept / with n_sel < E
void expect(bool ok, const char* what, const Case& c, uint32_t s, uint32_t feat) {
    if (ok) return;
    std::fprintf(stderr, "FAILED %s: case '%s', station %u, FEAT %#x\n", what, c.name, s, feat);
    g_failed += 1;
}

// the selection restated: eligible = key < kHi, in time order; the first min(E, room, 64) go to the lanes, the rest stay in list order
template <uint32_t FEAT>
void check(const Case& c, uint32_t s) {
    const unsigned long long ranked_before = aff::g_select_window_by_list[s][0], bucket_before = aff::g_select_window_by_list[s][1];
    const unsigned long long kept_before = aff::g_select_window_calls[2], short_before = aff::g_select_window_calls[3];
    const Result r = run_select<FEAT>(c, s);
    const uint32_t n = (uint32_t)c.key.size();
    const bool has_aux = s == 2u || ((FEAT & aff::FEAT_FAR) != 0u && s == 3u);
    bool ranked_call = false;   // the window must rank this call
    {
        // the path at the width of THIS list: the window ranks the call iff every eligible entry is later than every eligible
        // entry more than `width` lanes in front of it (the keys of the cases are far enough apart to have distinct codes)
        const uint32_t width = aff::select_window_of(s);
        bool proved = true;
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = 0; j + width < i; ++j)
                if (c.key[i] < kHi && c.key[j] < kHi && !(c.key[j] < c.key[i])) proved = false;
        const unsigned long long ranked = aff::g_select_window_by_list[s][0] - ranked_before, bucket = aff::g_select_window_by_list[s][1] - bucket_before;
        const bool called = width != 0u && n != 0u;   // (an empty list returns before the rank; no window, no count)
        expect(ranked == (called && proved ? 1ull : 0ull) && bucket == (called && !proved ? 1ull : 0ull), "path taken at this list's width", c, s, FEAT);
        ranked_call = called && proved;
    }
    expect((r.why & aff::FLOW_WHY_TIE) == 0u, "no tie", c, s, FEAT);
    std::printf("%s s=%u feat=%#x n_sel=%u kept=%u why=%#x H=%016llx", c.name, s, FEAT, r.n_sel, r.kept, r.why, (unsigned long long)bits(r.H));
    std::vector<uint32_t> el;
    for (uint32_t i = 0; i < n; ++i)
        if (c.key[i] < kHi) el.push_back(i);
    std::stable_sort(el.begin(), el.end(), [&](uint32_t a, uint32_t b) { return c.key[a] < c.key[b]; });
    const uint32_t E = (uint32_t)el.size(), n_sel = std::min(std::min(E, c.room), 64u);
    expect(r.n_sel == n_sel, "n_sel", c, s, FEAT);
    {
        // the branches behind a ranked call, from the emulator's counters: entries kept in the list, fewer selected than eligible
        const bool kept_some = ranked_call && n_sel < n, short_sel = ranked_call && n_sel < E;
        expect(aff::g_select_window_calls[2] - kept_before == (kept_some ? 1ull : 0ull), "ranked call counted as keeping entries", c, s, FEAT);
        expect(aff::g_select_window_calls[3] - short_before == (short_sel ? 1ull : 0ull), "ranked call counted as selecting fewer than eligible", c, s, FEAT);
        g_ranked_kept += kept_some ? 1 : 0;
        g_ranked_short += short_sel ? 1 : 0;
    }
    if (n != 0u) expect(bits(r.H) == bits(n_sel < E ? c.key[el[n_sel]] : kHi), "horizon", c, s, FEAT);
    std::vector<bool> taken(n, false);
    for (uint32_t k = 0; k < n_sel && k < r.n_sel; ++k) {
        taken[el[k]] = true;
        expect(bits(r.okey[k]) == bits(c.key[el[k]]) && bits(r.ot0[k]) == bits(t0_of(el[k])) && r.oaux[k] == (has_aux ? aux_of(el[k]) : 0u), "selected entry", c, s, FEAT);
    }
    for (uint32_t l = n_sel; l < 64u; ++l) expect(r.okey[l] == af::AF_INF && r.ot0[l] == 0.0 && r.oaux[l] == 0u, "idle lane", c, s, FEAT);
    uint32_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (taken[i]) continue;
        expect(pos < r.kept && bits(r.lkey[pos]) == bits(c.key[i]) && bits(r.lt0[pos]) == bits(t0_of(i)) && r.laux[pos] == (has_aux ? aux_of(i) : 0u), "kept entry", c, s, FEAT);
        pos += 1;
    }
    expect(pos == r.kept, "kept count", c, s, FEAT);
    for (uint32_t l = 0; l < 64u; ++l) std::printf(" %016llx:%016llx:%x", (unsigned long long)bits(r.okey[l]), (unsigned long long)bits(r.ot0[l]), r.oaux[l]);
    for (uint32_t i = 0; i < r.kept; ++i) std::printf(" %016llx:%016llx:%x", (unsigned long long)bits(r.lkey[i]), (unsigned long long)bits(r.lt0[i]), r.laux[i]);
    std::printf("\n");
}

std::vector<double> sorted_keys(uint32_t n) {
    std::vector<double> k(n);
    for (uint32_t i = 0; i < n; ++i) k[i] = kLo + (i + 0.5) * (0.9 / 64.0);
    return k;
}

}  // namespace

// select_widths --widths: this build's four widths; no argument: the cases
int main(int argc, char** argv) {
    static_assert(aff::select_window_of(0u) <= kWidest && aff::select_window_of(1u) <= kWidest && aff::select_window_of(2u) <= kWidest && aff::select_window_of(3u) <= kWidest,
                  "the crafted lists assume windows of at most eight lanes");
    const bool any_window = aff::select_window_of(0u) + aff::select_window_of(1u) + aff::select_window_of(2u) + aff::select_window_of(3u) != 0u;
    if (argc > 1 && std::strcmp(argv[1], "--widths") == 0) {
        std::printf("%u %u %u %u\n", aff::select_window_of(0u), aff::select_window_of(1u), aff::select_window_of(2u), aff::select_window_of(3u));
        return 0;
    }
    std::vector<Case> cases;
    cases.push_back({"empty list", {}, 64u});
    cases.push_back({"one entry", sorted_keys(1), 64u});
    cases.push_back({"one entry that stays", {kBeyond}, 64u});
    {
        auto k = sorted_keys(63);
        std::swap(k[61], k[62]);
        cases.push_back({"63 entries, all go", k, 64u});
    }
    cases.push_back({"64 sorted entries, all go", sorted_keys(64), 64u});
    {
        auto k = sorted_keys(64);
        for (uint32_t i = 0; i + 1u < 64u; i += 2u) std::swap(k[i], k[i + 1u]);
        cases.push_back({"64 entries, every pair swapped, all go", k, 64u});
    }
    {
        auto k = sorted_keys(64);
        std::swap(k[29], k[30]);   // the first entry left behind sits in front of one that goes
        cases.push_back({"room for fewer than are eligible", k, 30u});
    }
    {
        auto k = sorted_keys(64);
        std::swap(k[0], k[1]);
        cases.push_back({"room for one", k, 1u});
    }
    {
        auto k = sorted_keys(64);
        std::swap(k[0], k[1]);
        cases.push_back({"no room", k, 0u});
    }
    {
        auto k = sorted_keys(64);
        for (uint32_t i = 0; i < 64u; i += 3u) k[i] = kBeyond + i;
        std::swap(k[7], k[8]);
        cases.push_back({"eligible and other entries interleaved", k, 64u});
    }
    {
        auto k = sorted_keys(64);
        for (uint32_t i = 0; i < 64u; i += 2u) k[i] = kBeyond + i;
        cases.push_back({"eligible and other entries interleaved, room for ten", k, 10u});
    }
    {
        auto k = sorted_keys(64);
        for (uint32_t i = 0; i < 64u; ++i) k[i] = i < 40u ? kBeyond + i : k[i];
        cases.push_back({"nothing eligible in the first forty lanes", k, 64u});
    }
    {
        auto k = sorted_keys(64);
        for (uint32_t i = 0; i < 64u; ++i) k[i] = kBeyond + i;
        cases.push_back({"nothing eligible at all", k, 64u});
    }
    {
        auto k = sorted_keys(64);
        std::swap(k[20], k[23]);   // three lanes apart: ranked by a window of three or more, by the bucket rank below that
        cases.push_back({"inversion three lanes apart", k, 64u});
    }
    {
        auto k = sorted_keys(64);
        std::swap(k[20], k[21 + kWidest]);   // further apart than any window of the test: the bucket rank
        cases.push_back({"inversion wider than every window", k, 64u});
    }
    {
        auto k = sorted_keys(64);
        std::swap(k[5], k[6 + kWidest]);
        for (uint32_t i = 40u; i < 64u; i += 2u) k[i] = kBeyond + i;
        cases.push_back({"inversion wider than every window, room for seven, entries that stay", k, 7u});
    }
    const unsigned long long* g = aff::g_select_window_calls;
    for (const Case& c : cases) {
        check<0u>(c, 0u);
        check<0u>(c, 1u);
        check<0u>(c, 2u);
        check<0u>(c, 3u);
        check<aff::FEAT_FAR>(c, 2u);
        check<aff::FEAT_FAR>(c, 3u);
        check<aff::FEAT_MARKS>(c, 1u);
    }
    // both ranks ran in a build that has the window at all
    if (any_window ? (g[0] == 0ull || g[1] == 0ull) : (g[0] != 0ull || g[1] != 0ull)) {
        std::fprintf(stderr, "FAILED: calls ranked by the window %llu, by the bucket rank %llu\n", g[0], g[1]);
        g_failed += 1;
    }
    // ... and, of the ranked calls, some kept entries in the list and some selected fewer than were eligible: each branch at
    // least once, by the cases' own reckoning and by the emulator's counters
    if (any_window && (g[2] == 0ull || g[3] == 0ull || g_ranked_kept == 0 || g_ranked_short == 0 || g[2] != (unsigned long long)g_ranked_kept ||
                       g[3] != (unsigned long long)g_ranked_short)) {
        std::fprintf(stderr, "FAILED: ranked calls with entries kept %llu (cases: %d), with fewer selected than eligible %llu (cases: %d)\n", g[2], g_ranked_kept, g[3], g_ranked_short);
        g_failed += 1;
    }
    if (g_failed != 0) {
        std::fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    std::fprintf(stderr, "select_widths: %zu cases x 7 forms, widths %u %u %u %u: ranked by the window %llu (entries kept %llu, n_sel < E %llu), by the bucket rank %llu: ok\n", cases.size(),
                 aff::select_window_of(0u), aff::select_window_of(1u), aff::select_window_of(2u), aff::select_window_of(3u), g[0], g[2], g[3], g[1]);
    return 0;
}
