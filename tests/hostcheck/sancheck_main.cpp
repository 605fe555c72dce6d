// sancheck_main.cpp -- TEST-ONLY stand-alone program around hostcheck.cpp for AddressSanitizer / UBSan runs.
//
//     sancheck <case file> <result file>      run one case (tests/hostcheck/cases.py writes the case and reads the result)
//     sancheck --selfcheck                    prove that the instrumentation is live
//
// The -O2 library is loaded into Python and cannot be looked at by a sanitizer there; this program is the same source with a
// main of its own, run as a child process.  Every buffer a kernel is given -- clock, samples, counts, overrides, online
// arrays, every array of the plan -- is a heap allocation of its own of exactly the size the kernel is told, so a redzone
// sits right behind the last legal element; hc_flow_simulate's LDS block and hc_simulate's state words are exact likewise.
// Built by tests/hostcheck/build.py::build_sanitized only.
#if !defined(__SANITIZE_ADDRESS__)
#error "sancheck_main.cpp is for -fsanitize=address builds only (tests/hostcheck/build.py::build_sanitized)"
#endif
#include <sanitizer/asan_interface.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "hostcheck.cpp"

namespace {

// a case / result file is a sequence of 8-byte little-endian words: scalars one word each (integers as int64, reals as f64),
// arrays as a length word followed by one word per element
struct Reader {
    std::vector<uint64_t> w;
    size_t at = 0;
    uint64_t word() {
        if (at >= w.size()) {
            std::fprintf(stderr, "sancheck: case file too short\n");
            std::exit(3);
        }
        return w[at++];
    }
    int64_t i() { return (int64_t)word(); }
    double d() {
        const uint64_t v = word();
        double x;
        std::memcpy(&x, &v, 8);
        return x;
    }
    // an allocation of exactly n elements (n == 0: a zero-sized one, still a pointer of its own)
    template <class T>
    std::unique_ptr<T[]> ints(uint32_t* n_out = nullptr) {
        const size_t n = (size_t)word();
        std::unique_ptr<T[]> a(new T[n]);
        for (size_t k = 0; k < n; ++k) a[k] = (T)i();
        if (n_out) *n_out = (uint32_t)n;
        return a;
    }
    std::unique_ptr<double[]> reals(uint32_t* n_out = nullptr) {
        const size_t n = (size_t)word();
        std::unique_ptr<double[]> a(new double[n]);
        for (size_t k = 0; k < n; ++k) a[k] = d();
        if (n_out) *n_out = (uint32_t)n;
        return a;
    }
};

template <class T>
std::unique_ptr<T[]> zeros(size_t n) {
    std::unique_ptr<T[]> a(new T[n]);
    for (size_t k = 0; k < n; ++k) a[k] = T(0);
    return a;
}

struct Writer {
    std::FILE* f;
    void word(uint64_t v) { std::fwrite(&v, 8, 1, f); }
    template <class T>
    void raw(const T* p, size_t n) {   // length word, then the elements as they lie in memory
        word(n);
        if (n) std::fwrite(p, sizeof(T), n, f);
    }
};

int selfcheck() {
    // shadow queries only: nothing here touches the bytes it asks about
    const size_t lds_words = 2048u + 3333u, clock_rows = 777u;
    std::unique_ptr<uint64_t[]> lds(new uint64_t[lds_words]);
    std::unique_ptr<double[]> clock(new double[2u * clock_rows]);
    const int in_lds = __asan_address_is_poisoned(lds.get() + lds_words - 1u);
    const int past_lds = __asan_address_is_poisoned(lds.get() + lds_words);
    const int in_clock = __asan_address_is_poisoned(clock.get() + 2u * clock_rows - 1u);
    const int past_clock = __asan_address_is_poisoned(clock.get() + 2u * clock_rows);
    std::printf("selfcheck: lds last word poisoned=%d, word behind the lds block poisoned=%d\n", in_lds, past_lds);
    std::printf("selfcheck: clock last word poisoned=%d, word behind the clock buffer poisoned=%d\n", in_clock, past_clock);
    return (!in_lds && past_lds && !in_clock && past_clock) ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "--selfcheck") == 0) return selfcheck();
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <case file> <result file> | --selfcheck\n", argv[0]);
        return 2;
    }
    Reader r;
    {
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f) {
            std::perror(argv[1]);
            return 2;
        }
        uint64_t v;
        while (std::fread(&v, 8, 1, f) == 1) r.w.push_back(v);
        std::fclose(f);
    }
    if (r.word() != 0x3153414346415341ull /* "ASAFCAS1" */) {
        std::fprintf(stderr, "sancheck: not a case file\n");
        return 2;
    }
    const int64_t mode = r.i();   // 0 next-event lane (hc_simulate), 1 flow kernel (hc_flow_simulate), 2 arrival sampler (hc_arrivals)

    // ---- the plan -------------------------------------------------------------------------------------------------------
    af_plan_t p{};
    p.abi_version = AF_ABI_VERSION;
    p.struct_size = sizeof(af_plan_t);
    p.total_time = r.d();
    p.sample_period = r.d();
    p.metrics_mask = (uint32_t)r.i();
    p.gen_users_dist = (uint32_t)r.i();
    p.gen_users_mean = r.d();
    p.gen_users_sigma = r.d();
    p.gen_rpm_mean = r.d();
    p.gen_window_s = r.d();
    p.gen_out_edge = (int32_t)r.i();
    p.n_edges = (uint32_t)r.i();
    p.n_servers = (uint32_t)r.i();
    p.client_out_edge = (int32_t)r.i();
    p.has_lb = (uint32_t)r.i();
    p.lb_algo = (uint32_t)r.i();
    const auto lb_edges = r.ints<int32_t>(&p.n_lb_edges);
    const auto edge_target_kind = r.ints<uint8_t>();
    const auto edge_target_idx = r.ints<int32_t>();
    const auto edge_dist = r.ints<uint8_t>();
    const auto edge_mean = r.reals();
    const auto edge_sigma = r.reals();
    const auto edge_dropout = r.reals();
    const auto srv_cores = r.ints<uint32_t>();
    const auto srv_ram_mb = r.reals();
    const auto srv_out_edge = r.ints<int32_t>();
    const auto srv_ep_begin = r.ints<uint32_t>();
    const auto ep_step_begin = r.ints<uint32_t>();
    const auto ep_ram = r.reals(&p.n_endpoints);
    const auto step_kind = r.ints<uint8_t>(&p.n_steps);
    const auto step_time = r.reals();
    const auto emark_time = r.reals(&p.n_edge_marks);
    const auto emark_edge = r.ints<int32_t>();
    const auto emark_delta = r.reals();
    const auto smark_time = r.reals(&p.n_srv_marks);
    const auto smark_lb_edge = r.ints<int32_t>();
    const auto smark_down = r.ints<uint8_t>();
    p.lb_edges = lb_edges.get();
    p.edge_target_kind = edge_target_kind.get();
    p.edge_target_idx = edge_target_idx.get();
    p.edge_dist = edge_dist.get();
    p.edge_mean = edge_mean.get();
    p.edge_sigma = edge_sigma.get();
    p.edge_dropout = edge_dropout.get();
    p.srv_cores = srv_cores.get();
    p.srv_ram_mb = srv_ram_mb.get();
    p.srv_out_edge = srv_out_edge.get();
    p.srv_ep_begin = srv_ep_begin.get();
    p.ep_step_begin = ep_step_begin.get();
    p.ep_ram = ep_ram.get();
    p.step_kind = step_kind.get();
    p.step_time = step_time.get();
    p.emark_time = emark_time.get();
    p.emark_edge = emark_edge.get();
    p.emark_delta = emark_delta.get();
    p.smark_time = smark_time.get();
    p.smark_lb_edge = smark_lb_edge.get();
    p.smark_down = smark_down.get();

    // ---- the scenario and the knobs ---------------------------------------------------------------------------------------
    const uint64_t seed = r.word();
    uint32_t n_ovr = 0;
    const auto ovr_param = r.ints<uint32_t>(&n_ovr);
    const auto ovr_index = r.ints<uint32_t>();
    const auto ovr_value = r.reals();
    const int two_pass = (int)r.i();
    const uint32_t ipl = (uint32_t)r.i(), ring_rows = (uint32_t)r.i();
    const bool robust = r.i() != 0, far = r.i() != 0, compact = r.i() != 0;
    const uint32_t long_list_entries = (uint32_t)r.i();
    const int64_t long_list = r.i();   // -1: all four lists
    const uint32_t cap = (uint32_t)r.i(), fcap = (uint32_t)r.i();
    const uint32_t clock_cap = (uint32_t)r.i(), draw_cap = (uint32_t)r.i(), tick_cap = (uint32_t)r.i();
    const bool with_samples = r.i() != 0;
    const uint32_t hist_bins = (uint32_t)r.i();
    const double hist_max = r.d();
    const uint32_t rps_buckets = (uint32_t)r.i();
    const int quantum_bits = (int)r.i();
    // hc_arrivals
    const int which = (int)r.i();
    const uint32_t a_dist = (uint32_t)r.i();
    const double a_mean = r.d(), a_sigma = r.d(), a_rpm = r.d(), a_window = r.d(), a_horizon = r.d();
    const uint32_t a_n_draw = (uint32_t)r.i();
    if (r.at != r.w.size()) {
        std::fprintf(stderr, "sancheck: %zu words left over in the case file\n", r.w.size() - r.at);
        return 2;
    }

    const uint32_t pitch = (p.n_edges + 3u * p.n_servers + 3u) & ~3u;
    const auto clock = zeros<double>((size_t)clock_cap * 2u);
    const auto samples = zeros<uint32_t>(with_samples ? (size_t)tick_cap * pitch : 0u);
    const auto counts = zeros<uint32_t>(AF_CNT_SLOTS);
    const auto hist = zeros<uint32_t>(hist_bins);
    const auto rps = zeros<uint32_t>(rps_buckets);
    const auto arrivals = zeros<double>(mode == 2 ? a_n_draw : 0u);
    uint32_t arr_flags = 0;
    int64_t rc = 0, arr_n = 0;

    hc_set_test_quantum(quantum_bits);
    hc_set_two_pass(two_pass);
    hc_set_online(hist_bins ? hist.get() : nullptr, hist_bins, hist_max, rps_buckets ? rps.get() : nullptr, rps_buckets);
    if (mode == 0) {
        rc = hc_simulate(&p, seed, n_ovr, ovr_param.get(), ovr_index.get(), ovr_value.get(), cap, fcap, clock_cap, clock.get(), tick_cap,
                         with_samples ? samples.get() : nullptr, counts.get(), draw_cap);
    } else if (mode == 1) {
        const uint32_t word = ipl | (far ? 0u : 0x200u) | (compact ? 0x400u : 0u) |
                              (robust ? (0x100u | (long_list_entries << 16) | ((uint32_t)(long_list + 1) << 12)) : 0u);
        rc = hc_flow_simulate(&p, seed, n_ovr, ovr_param.get(), ovr_index.get(), ovr_value.get(), word, ring_rows, clock_cap, clock.get(),
                              tick_cap, with_samples ? samples.get() : nullptr, counts.get(), draw_cap);
    } else if (mode == 2) {
        arr_n = hc_arrivals(which, seed, a_dist, a_mean, a_sigma, a_rpm, a_window, a_horizon, a_n_draw, arrivals.get(), &arr_flags);
    } else {
        std::fprintf(stderr, "sancheck: unknown mode\n");
        return 2;
    }

    std::FILE* f = std::fopen(argv[2], "wb");
    if (!f) {
        std::perror(argv[2]);
        return 2;
    }
    Writer o{f};
    o.word((uint64_t)rc);
    o.word((uint64_t)(int64_t)(mode == 1 ? hc_flow_variant() : mode == 0 ? hc_sim_variant() : which));
    o.word((uint64_t)arr_n);
    o.word(arr_flags);
    o.raw(counts.get(), AF_CNT_SLOTS);
    o.raw(clock.get(), (size_t)clock_cap * 2u);
    o.raw(samples.get(), with_samples ? (size_t)tick_cap * pitch : 0u);
    o.raw(hist.get(), hist_bins);
    o.raw(rps.get(), rps_buckets);
    o.raw(arrivals.get(), mode == 2 ? a_n_draw : 0u);
    return std::fclose(f) == 0 ? 0 : 2;
}
