// sequence_counts_sanitize.cpp -- dig_sequence_counts_host and a plain statement of it in one stand-alone program for a host
// sanitizer build: the cases of tests/test_gpu_sequence_models.py that stress the pair list -- cohort boundaries inside a wave, an
// empty cohort, a cohort without pairs, one counter past 65 535 at K = 192 and K = 3 072, and a row whose 300 pairs span waves and
// workgroups.  The pair list is made here by a brute-force join, as dig_overlap_join_fill orders it (row-major).
//
// In a copy of the tree (the objects must not end up in the product's library):
//   make -C digdriver_amd/csrc -j8 OUT=/tmp/libdig_san.so EXTRA="-g -Xarch_host -fsanitize=address,undefined"
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fsanitize=address,undefined digdriver_amd/csrc/*.o \
//       tools/sequence_counts_sanitize.cpp -o /tmp/sequence_counts_sanitize && /tmp/sequence_counts_sanitize
//
// The twin checks its arrays on the host and then stages them through a card.  Without a card the program still runs the checks,
// the staging's failure path and the statement under the sanitizers, says so, and exits 0; with one it compares the counts.
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../include/dig_hip.h"

namespace {

struct Window {
    int64_t chrom, start, end;
};
struct Rows {
    std::vector<int64_t> chrom, start;
    std::vector<int32_t> type, cohort;
    void add(int64_t c, int64_t s, int32_t t, int32_t k)
    {
        chrom.push_back(c), start.push_back(s), type.push_back(t), cohort.push_back(k);
    }
};

int run(const char* name, const std::vector<Window>& win, const Rows& rows, int64_t K, int64_t C)
{
    const int64_t n = (int64_t)rows.type.size();
    std::vector<int32_t> pair_row;
    std::vector<int64_t> want((size_t)(C * K), 0), got((size_t)(C * K), -1);
    for (int64_t r = 0; r < n; ++r) {
        bool hit = false;
        for (const Window& w : win)
            if (w.chrom == rows.chrom[r] && w.start <= rows.start[r] && rows.start[r] < w.end) pair_row.push_back((int32_t)r), hit = true;
        if (hit && rows.type[r] < K) want[(size_t)(rows.cohort[r] * K + rows.type[r])] += 1;
    }
    const int rc = dig_sequence_counts_host(pair_row.data(), (int64_t)pair_row.size(), rows.type.data(), rows.cohort.data(), n, K, C,
                                            got.data(), 0);
    if (rc == DIG_EHIP) {
        printf("%s: %lld rows, %lld pairs: host checks passed; no device here (%s)\n", name, (long long)n, (long long)pair_row.size(),
               dig_last_error());
        return 0;
    }
    if (rc != DIG_OK) {
        printf("%s: refused: %s\n", name, dig_last_error());
        return 1;
    }
    int64_t largest = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        if (got[i] != want[i]) {
            printf("%s: counter %zu is %lld, the statement says %lld\n", name, i, (long long)got[i], (long long)want[i]);
            return 1;
        }
        if (want[i] > largest) largest = want[i];
    }
    printf("%s: %lld rows, %lld pairs: equal to the statement (largest counter %lld)\n", name, (long long)n, (long long)pair_row.size(),
           (long long)largest);
    return 0;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(5);
    auto below = [&](int64_t m) { return (int64_t)(rng() % (uint64_t)m); };
    const std::vector<Window> win = {{1, 0, 100}, {1, 100, 200}, {1, 150, 260}, {1, 400, 500}, {1, 400, 500}, {2, 0, 1000}};
    int bad = 0;
    {   // 287 rows: cohort 0 ends inside a wave, cohort 1 is empty, cohort 3 has rows and no pair
        Rows r;
        for (int i = 0; i < 100; ++i) r.add(1, below(260), (int32_t)below(193), 0);
        for (int i = 0; i < 150; ++i) r.add(1, 100 + below(400), (int32_t)below(193), 2);
        for (int i = 0; i < 37; ++i) r.add(i < 20 ? 1 : 3, i < 20 ? 260 + below(140) : below(100), (int32_t)below(192), 3);
        bad += run("cohort boundaries", win, r, 192, 4);
    }
    for (int64_t K : {192, 3072}) {   // 70 000 rows of one type and 5 000 over all types, one cohort
        Rows r;
        for (int i = 0; i < 75000; ++i) r.add(2, below(1000), i % 15 ? (int32_t)(K / 3 + 1) : (int32_t)((i / 15) % K), 0);
        bad += run(K == 192 ? "one hot counter, K = 192" : "one hot counter, K = 3072", win, r, K, 1);
    }
    {   // the last row of cohort 0 lies in 300 copies of a window behind 900 one-pair rows; the first row of cohort 1 in the same
        std::vector<Window> many(300, Window{1, 0, 1000});
        many.push_back({1, 2000, 3000});
        Rows r;
        for (int i = 0; i < 900; ++i) r.add(1, 2000 + i, i % 192, 0);
        r.add(1, 500, 7, 0);
        r.add(1, 600, 7, 1);
        r.add(1, 2500, 8, 1);
        r.add(1, 700, 192, 1);
        bad += run("a row's pairs across workgroups", many, r, 192, 2);
    }
    // the twin's refusals
    const int32_t t[2] = {0, 5}, c[2] = {0, 1}, p[2] = {0, 1};
    int64_t out[16];
    bad += dig_sequence_counts_host(p, 2, t, c, 2, 0, 2, out, 0) != DIG_EINVAL;
    bad += dig_sequence_counts_host(p, 2, t, c, 2, 5, 1, out, 0) != DIG_EINVAL;
    bad += dig_sequence_counts_host(p, 2, t, c, 2, 4, 2, out, 0) != DIG_EINVAL;
    printf(bad ? "FAILED\n" : "done\n");
    return bad != 0;
}
