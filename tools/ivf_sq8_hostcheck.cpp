// ivf_sq8_hostcheck.cpp — the pure host functions of the IVF SQ8 stages (csrc/ivf_sq8_host.hpp) under the host
// sanitizers, as a stand-alone program:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ivf_sq8_hostcheck.cpp -o hostcheck
//   ./hostcheck
#include "../duckdb-annsearch_amd/csrc/ivf_sq8_host.hpp"

#include <cstdio>
#include <cstring>
#include <limits>

using namespace hipann;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
    const int d = 33, nlist = 4;
    std::vector<float> cen((size_t)nlist * d, 1.f), vmin(d, -2.f), vdiff(d, 255.f);
    std::vector<int64_t> off = {0, 0, 31, 2080, 6177}, ids(6177);
    std::vector<uint8_t> codes((size_t)6177 * d, 7);
    auto create = [&]() {
        return ivf_sq_check_create(d, 0, nlist, 1, cen.data(), vmin.data(), vdiff.data(), off.data(), ids.data(),
                                   codes.data());
    };
    CHECK(create() == nullptr);
    vdiff[5] = std::numeric_limits<float>::quiet_NaN();
    CHECK(create() && std::strstr(create(), "finite"));
    vdiff[5] = 255.f;
    off[2] = -1;
    CHECK(create() && std::strstr(create(), "ascending"));
    off[2] = 31;
    CHECK(ivf_sq_check_create(0, 0, nlist, 1, cen.data(), vmin.data(), vdiff.data(), off.data(), ids.data(), codes.data()));
    CHECK(ivf_sq_check_create(d, 2, nlist, 1, cen.data(), vmin.data(), vdiff.data(), off.data(), ids.data(), codes.data()));
    CHECK(ivf_sq_check_create(d, 0, nlist, 1, cen.data(), vmin.data(), vdiff.data(), off.data(), nullptr, codes.data()));
    CHECK(ivf_sq_check_search(3, 0, 2048, true) && ivf_sq_check_search(3, 2049, 2048, true));
    CHECK(ivf_sq_check_search(3, 1, 2048, false) && !ivf_sq_check_search(0, 1, 2048, false));
    CHECK(ivf_sq_call_nprobe(0, 3, 4) == 3 && ivf_sq_call_nprobe(9, 3, 4) == 4 && ivf_sq_call_nprobe(2, 3, 4) == 2);
    const std::vector<float> sb = ivf_sq_scale_bias(vmin.data(), vdiff.data(), d, 128);
    CHECK(sb.size() == 256 && sb[0] == 1.f && sb[128] == -1.5f && sb[d] == 0.f && sb[128 + d] == 0.f);
    double gmax = 0, mnorm = 0;
    ivf_sq_magnitudes(cen.data(), nlist, d, true, vmin.data(), vdiff.data(), &gmax, &mnorm);
    CHECK(std::fabs(gmax - std::sqrt(33.0)) < 1e-12 && mnorm > 255.0 * std::sqrt(33.0));
    ivf_sq_magnitudes(cen.data(), nlist, d, false, vmin.data(), vdiff.data(), &gmax, &mnorm);
    CHECK(gmax == 0.0);
    const std::vector<int64_t> tp = ivf_sq_pass_offsets(off.data(), nlist);
    CHECK(tp.size() == 5 && tp[1] == 0 && tp[2] == 1 && tp[3] == 66 && tp[4] == 66 + 129);
    const std::vector<int64_t> len = {0, 31, 2049, 4097};
    CHECK(ivf_sq_query_slots(len, 1, 2048) == 3 && ivf_sq_query_slots(len, 2, 2048) == 5);
    CHECK(ivf_sq_query_slots(len, 9, 2048) == 6 && ivf_sq_query_slots({0, 0}, 2, 2048) == 1);
    CHECK(ivf_sq_slice_queries(1000, 6, 1536, 256 << 20) == 1000 && ivf_sq_slice_queries(1000, 64, 16384, 1 << 20) == 1);
    // hipann_ivfsq_remove_ids: the label set and the length bookkeeping
    const int64_t raw[] = {9, -3, 9, 1LL << 40, -3, 0};
    CHECK((ivf_sq_label_set(raw, 6) == std::vector<int64_t>{-3, 0, 9, 1LL << 40}) && ivf_sq_label_set(raw, 0).empty());
    std::vector<int64_t> cur = len;
    const int after[] = {0, 30, 2049, 0}, over[] = {0, 32, 2049, 0}, neg[] = {0, 31, -1, 0};
    CHECK(ivf_sq_removed_lengths(cur, over) == -1 && ivf_sq_removed_lengths(cur, neg) == -1 && cur == len);
    CHECK(ivf_sq_removed_lengths(cur, after) == 4098 && (cur == std::vector<int64_t>{0, 30, 2049, 0}));
    std::printf(fails ?"%d checks failed\n" : "ivf_sq8 host checks passed\n", fails);
    return fails ? 1 : 0;
}
