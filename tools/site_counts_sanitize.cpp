// site_counts_sanitize.cpp -- the three site-match twins (dig_site_match_count_host, dig_site_match_keys_host, dig_site_counts_host)
// and a plain statement of them in one stand-alone program for a host sanitizer build: equal-position runs, rows below the first and
// above the last site, negative attr, a site row listed twice, runs of one (element, sample) across wave and workgroup boundaries,
// empty inputs, and the twins' refusals.
//
// In a copy of the tree (the objects must not end up in the product's library):
//   make -C digdriver_amd/csrc -j8 OUT=/tmp/libdig_san.so EXTRA="-g -Xarch_host -fsanitize=address,undefined"
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -fsanitize=address,undefined digdriver_amd/csrc/*.o \
//       tools/site_counts_sanitize.cpp -o /tmp/site_counts_sanitize && /tmp/site_counts_sanitize
//
// The twins check their arrays on the host and then stage them through a card.  Without a card the program still runs the checks,
// the staging's failure path and the statement under the sanitizers, says so, and exits 0; with one it compares the counts.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../include/dig_hip.h"

namespace {

struct Site {
    int64_t pos, end, attr;
    int32_t elt;
    bool operator<(const Site& o) const { return pos < o.pos; }
};
struct Rows {
    std::vector<int64_t> pos, end, attr;
    std::vector<int32_t> sample, cohort;
    void add(int64_t p, int64_t e, int64_t a, int32_t s, int32_t c)
    {
        pos.push_back(p), end.push_back(e), attr.push_back(a), sample.push_back(s), cohort.push_back(c);
    }
};

int run(const char* name, std::vector<Site> sites, const Rows& rows, int64_t E, const std::vector<int64_t>& off)
{
    std::stable_sort(sites.begin(), sites.end());
    const int64_t S = (int64_t)sites.size(), n = (int64_t)rows.pos.size(), C = (int64_t)off.size() - 1, n_samples = off.back();
    std::vector<int64_t> sp, se, sa;
    std::vector<int32_t> sl;
    for (const Site& s : sites) sp.push_back(s.pos), se.push_back(s.end), sa.push_back(s.attr), sl.push_back(s.elt);
    // the statement: every (row, site) pair, then per (element, cohort) the pairs and the distinct samples
    std::vector<int32_t> want_snv((size_t)(E * C), 0), want_samples((size_t)(E * C), 0), want_counts((size_t)n, 0);
    std::vector<std::vector<int32_t>> seen((size_t)(E * C));
    for (int64_t i = 0; i < n; ++i)
        for (const Site& s : sites)
            if (rows.attr[i] >= 0 && s.pos == rows.pos[i] && s.end == rows.end[i] && s.attr == rows.attr[i]) {
                const size_t at = (size_t)(s.elt * C + rows.cohort[i]);
                want_counts[(size_t)i] += 1, want_snv[at] += 1, seen[at].push_back(rows.sample[i]);
            }
    for (size_t at = 0; at < seen.size(); ++at) {
        std::sort(seen[at].begin(), seen[at].end());
        want_samples[at] = (int32_t)(std::unique(seen[at].begin(), seen[at].end()) - seen[at].begin());
    }
    std::vector<int32_t> counts((size_t)n, -7);
    int rc = dig_site_match_count_host(sp.data(), se.data(), sa.data(), sl.data(), S, E, rows.pos.data(), rows.end.data(), rows.attr.data(),
                                       rows.sample.data(), rows.cohort.data(), off.data(), n, C, n_samples, counts.data(), 0);
    const bool no_card = rc == DIG_EHIP;
    if (rc != DIG_OK && !no_card) return printf("%s: count refused: %s\n", name, dig_last_error()), 1;
    if (no_card) counts = want_counts;                    // (the later twins still check their arrays)
    if (counts != want_counts) return printf("%s: the counts differ from the statement\n", name), 1;
    std::vector<int64_t> offsets((size_t)n, 0);
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) offsets[(size_t)i] = total, total += counts[(size_t)i];
    std::vector<int64_t> keys((size_t)total, 0);
    rc = dig_site_match_keys_host(sp.data(), se.data(), sa.data(), sl.data(), S, E, rows.pos.data(), rows.end.data(), rows.attr.data(),
                                  rows.sample.data(), rows.cohort.data(), off.data(), n, C, n_samples, offsets.data(), total, keys.data(), 0);
    if (rc != DIG_OK && rc != DIG_EHIP) return printf("%s: keys refused: %s\n", name, dig_last_error()), 1;
    std::sort(keys.begin(), keys.end());
    std::vector<int32_t> snv((size_t)(E * C), -7), samples((size_t)(E * C), -7);
    rc = dig_site_counts_host(keys.data(), total, E, C, n_samples, snv.data(), samples.data(), 0);
    if (rc != DIG_OK && rc != DIG_EHIP) return printf("%s: counts refused: %s\n", name, dig_last_error()), 1;
    if (no_card) {
        printf("%s: %lld rows, %lld sites, %lld matches: host checks passed; no device here (%s)\n", name, (long long)n, (long long)S,
               (long long)total, dig_last_error());
        return 0;
    }
    if (snv != want_snv || samples != want_samples) return printf("%s: the planes differ from the statement\n", name), 1;
    printf("%s: %lld rows, %lld sites, %lld matches: equal to the statement\n", name, (long long)n, (long long)S, (long long)total);
    return 0;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(9);
    auto below = [&](int64_t m) { return (int64_t)(rng() % (uint64_t)m); };
    int bad = 0;
    {   // 2 000 sites at 300 positions, 3 cohorts x 2 500 rows in any order, a tenth with a negative attr
        std::vector<Site> sites;
        for (int i = 0; i < 2000; ++i) sites.push_back({((int64_t)3 << 40) | (1000 + 7 * below(300)), 0, below(5), (int32_t)below(30)});
        for (Site& s : sites) s.end = s.pos + 1 + below(2);
        Rows r;
        const std::vector<int64_t> off = {0, 40, 40, 100};          // the second cohort has no sample and no row
        for (int i = 0; i < 7500; ++i) {
            const int32_t c = below(2) ? 0 : 2;
            const int64_t p = ((int64_t)3 << 40) | (993 + 7 * below(302));      // one position below the first site, one above the last
            r.add(p, p + 1 + below(2), below(10) ? below(5) : -1, (int32_t)(off[(size_t)c] + below(off[(size_t)c + 1] - off[(size_t)c])), c);
        }
        bad += run("fuzz", sites, r, 30, off);
    }
    {   // one site listed twice; 256 + 64 + 1 rows of one sample, then runs that start at key 63 and 255 of the next element
        std::vector<Site> sites = {{10, 11, 0, 0}, {10, 11, 0, 0}, {20, 21, 0, 1}, {20, 22, 0, 1}, {20, 21, 1, 1}};
        Rows r;
        for (int i = 0; i < 161; ++i) r.add(10, 11, 0, 3, 0);       // 322 keys of (element 0, sample 3)
        for (int i = 0; i < 5; ++i) r.add(20, 21, 0, 0, 0);
        for (int i = 0; i < 300; ++i) r.add(20, 21, 0, (int32_t)(1 + i / 60), 0);
        r.add(20, 23, 0, 0, 0), r.add(19, 21, 0, 0, 0), r.add(21, 21, 0, 0, 0);
        bad += run("runs across waves", sites, r, 2, {0, 8});
    }
    bad += run("no rows", {{10, 11, 0, 0}}, Rows(), 1, {0, 0});
    {
        Rows r;
        r.add(10, 11, 0, 0, 0);
        bad += run("no sites", {}, r, 1, {0, 1});
        bad += run("no match", {{10, 12, 0, 0}}, r, 1, {0, 1});
    }
    // the twins' refusals
    const int64_t pos[2] = {5, 4}, end[2] = {6, 5}, attr[2] = {0, 0}, off[2] = {0, 2}, offsets[2] = {0, 1};
    const int32_t elt[2] = {0, 1}, sample[2] = {0, 2}, cohort[2] = {0, 0};
    int32_t counts[2], planes[4];
    int64_t keys[2];
    bad += dig_site_match_count_host(pos, end, attr, elt, 2, 2, pos, end, attr, sample, cohort, off, 1, 1, 2, counts, 0) != DIG_EINVAL;       // sites descending
    bad += dig_site_match_count_host(pos, end, attr, elt, 1, 1, pos, end, attr, sample, cohort, off, 2, 1, 2, counts, 0) != DIG_EINVAL;       // a sample outside its cohort
    bad += dig_site_match_count_host(pos, end, attr, elt + 1, 1, 1, pos, end, attr, sample, cohort, off, 1, 1, 2, counts, 0) != DIG_EINVAL;   // an element outside [0, E)
    bad += dig_site_match_keys_host(pos, end, attr, elt, 1, 1, pos, end, attr, sample, cohort, off, 1, 1, 2, offsets + 1, 0, keys, 0) != DIG_EINVAL;   // an offset past total
    bad += dig_site_counts_host(pos, 2, 2, 1, 2, planes, planes + 2, 0) != DIG_EINVAL;                                                       // keys descending
    bad += dig_site_counts_host(nullptr, 0, ((int64_t)1 << 31) - 1, 3, ((int64_t)1 << 31) - 1, planes, planes, 0) != DIG_EINVAL;              // 64 bits
    printf(bad ? "FAILED\n" : "done\n");
    return bad != 0;
}
