// select_window_main.cpp -- TEST-ONLY stand-alone program: Flow::select() of the stage-parallel kernel (asyncflow_amd/csrc/af_flow.hpp)
// on crafted station lists, on the 64-fibre wave emulator of tests/hostcheck.
//
// Built twice by tests/test_flow_select_window.py -- with the lane window (the default) and with -DAF_SELECT_WINDOW=0 -- and once
// more under AddressSanitizer + UBSan.  Every case is held to a scalar restatement of the selection (a stable sort of the
// eligible keys) and, in the window build, to the path it must take (aff::g_select_window_calls); the program prints one line per
// case with every output word, and the test holds the lines of the two builds to each other.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../../asyncflow_amd/csrc/af_plan_pack.hpp"
#include "../../asyncflow_amd/csrc/af_flow_host.hpp"
#include "../hostcheck/wave_emul.hpp"

namespace {

constexpr uint32_t D = AF_SELECT_WINDOW;
constexpr double kLo = 1.0, kHi = 2.0, kBeyond = 2.5;   // horizon of the station, bound of the call, a key that is not eligible
enum Path { WINDOW, BUCKET };

struct Case {
    const char* name;
    std::vector<double> key;
    uint32_t room;
    Path path;    // what the window build must do
    bool tie;     // FLOW_WHY_TIE expected
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
uint32_t aux_of(uint32_t i) { return (i * 7u + 3u) & 0x1FFu; }

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
void expect(bool ok, const char* what, const Case& c, uint32_t s, uint32_t feat) {
    if (ok) return;
    std::fprintf(stderr, "FAILED %s: case '%s', station %u, FEAT %#x\n", what, c.name, s, feat);
    g_failed += 1;
}

// the selection restated: eligible = key < kHi, in time order; the first min(E, room, 64) go to the lanes, the rest stay in list order
template <uint32_t FEAT>
void check(const Case& c, uint32_t s) {
    aff::g_select_window_calls[0] = aff::g_select_window_calls[1] = 0ull;
    const Result r = run_select<FEAT>(c, s);
    const uint32_t n = (uint32_t)c.key.size();
    const bool has_aux = s == 2u || ((FEAT & aff::FEAT_FAR) != 0u && s == 3u);
    if (D == 0u) expect(aff::g_select_window_calls[0] == 0ull && aff::g_select_window_calls[1] == 0ull, "no window in this build", c, s, FEAT);
    else expect(aff::g_select_window_calls[c.path == WINDOW ? 0 : 1] == 1ull && aff::g_select_window_calls[c.path == WINDOW ? 1 : 0] == 0ull, "path taken", c, s, FEAT);
    expect(((r.why & aff::FLOW_WHY_TIE) != 0u) == c.tie, "tie flag", c, s, FEAT);
    std::printf("%s s=%u feat=%#x n_sel=%u kept=%u why=%#x H=%016llx", c.name, s, FEAT, r.n_sel, r.kept, r.why, (unsigned long long)bits(r.H));
    if (!c.tie) {   // (with equal keys two entries share a rank and the scenario is handed back: the flag is the result)
        std::vector<uint32_t> el;
        for (uint32_t i = 0; i < n; ++i)
            if (c.key[i] < kHi) el.push_back(i);
        std::stable_sort(el.begin(), el.end(), [&](uint32_t a, uint32_t b) { return c.key[a] < c.key[b]; });
        const uint32_t E = (uint32_t)el.size(), n_sel = std::min(std::min(E, c.room), 64u);
        expect(r.n_sel == n_sel, "n_sel", c, s, FEAT);
        expect(bits(r.H) == bits(n_sel < E ? c.key[el[n_sel]] : kHi), "horizon", c, s, FEAT);
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
    }
    std::printf("\n");
}

std::vector<double> sorted_keys(uint32_t n) {
    std::vector<double> k(n);
    for (uint32_t i = 0; i < n; ++i) k[i] = kLo + (i + 0.5) * (0.9 / 64.0);
    return k;
}

}  // namespace

// select_window --width: prints this build's window; select_window [w]: the lists crafted around a window of w lanes (default:
// this build's own; the build without a window is handed the other build's, so that both run the same lists)
int main(int argc, char** argv) {
    // the distances are in LANES: the cases are written for any window up to 12
    static_assert(D <= 12u, "the crafted lists assume a window of at most 12 lanes");
    if (argc > 1 && std::strcmp(argv[1], "--width") == 0) {
        std::printf("%u\n", D);
        return 0;
    }
    const uint32_t W = argc > 1 ? (uint32_t)std::atoi(argv[1]) : D;
    if (W < 4u || W > 12u || (D != 0u && W != D)) {
        std::fprintf(stderr, "list width %u: not this build's window (%u), or outside 4 .. 12\n", W, D);
        return 2;
    }
    std::vector<Case> cases;
    cases.push_back({"sorted", sorted_keys(64), 64u, WINDOW, false});
    {
        auto k = sorted_keys(64);
        std::swap(k[20], k[20 + W]);
        cases.push_back({"inversion at the window's width", k, 64u, WINDOW, false});
    }
    {
        auto k = sorted_keys(64);
        std::swap(k[20], k[21 + W]);
        cases.push_back({"inversion one lane wider than the window", k, 64u, BUCKET, false});
    }
    {
        auto k = sorted_keys(64);
        std::swap(k[63 - W], k[63]);
        std::swap(k[0], k[1]);
        std::swap(k[15], k[16]);   // across the rows of sixteen lanes
        std::swap(k[30], k[33]);   // across the halves of the wave
        cases.push_back({"inversions at the rows' and the wave's edges", k, 64u, WINDOW, false});
    }
    {
        auto k = sorted_keys(64);
        k[31] = k[29];
        cases.push_back({"equal keys inside a window", k, 64u, BUCKET, true});
    }
    {
        auto k = sorted_keys(64);
        k[20 + W + 3u] = k[20];
        cases.push_back({"equal keys further apart than the window", k, 64u, BUCKET, true});
    }
    {
        auto k = sorted_keys(64);
        k[31] = k[30] + 1e-13;   // closer than the 32-bit code resolves, not equal
        std::swap(k[30], k[31]);
        cases.push_back({"distinct keys with one code", k, 64u, BUCKET, false});
    }
    {
        auto k = sorted_keys(64);
        std::swap(k[10], k[10 + W]);
        for (uint32_t i = 11; i < 10 + W; i += 2) k[i] = kBeyond;
        k[40] = kBeyond;
        cases.push_back({"entries that stay between the halves of an inversion", k, 64u, WINDOW, false});
    }
    {
        auto k = sorted_keys(64);
        std::swap(k[10], k[11 + W]);
        for (uint32_t i = 11; i < 11 + W; ++i) k[i] = kBeyond;
        cases.push_back({"only entries that stay between the halves of a wide inversion", k, 64u, BUCKET, false});
    }
    cases.push_back({"one entry", sorted_keys(1), 64u, WINDOW, false});
    {
        auto k = sorted_keys(63);
        std::swap(k[61], k[62]);
        cases.push_back({"63 entries", k, 64u, WINDOW, false});
    }
    {
        auto k = sorted_keys(64);
        std::swap(k[29], k[31]);   // the first entry left behind sits in front of two that go
        cases.push_back({"room for fewer than are eligible", k, 30u, WINDOW, false});
    }
    {
        auto k = sorted_keys(64);
        std::swap(k[5], k[6 + W]);
        cases.push_back({"room for fewer than are eligible, bucket rank", k, 7u, BUCKET, false});
    }
    {
        auto k = sorted_keys(64);
        for (uint32_t i = 0; i < 64u; ++i) k[i] = i < 40u ? kBeyond + i : k[i];
        cases.push_back({"nothing eligible in the first forty lanes", k, 64u, WINDOW, false});
    }
    {
        auto k = sorted_keys(64);
        k[0] = kLo;   // an entry AT the horizon: code 1, like every key the scale cannot tell from it
        cases.push_back({"entry at the horizon", k, 64u, WINDOW, false});
    }
    for (const Case& c : cases) {
        check<0u>(c, 1u);
        check<0u>(c, 2u);
        check<aff::FEAT_FAR>(c, 2u);
        check<aff::FEAT_FAR>(c, 3u);
    }
    if (g_failed != 0) {
        std::fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    std::fprintf(stderr, "select_window: %zu cases x 4 forms, window %u: ok\n", cases.size(), D);
    return 0;
}
