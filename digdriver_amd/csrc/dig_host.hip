// dig_host.hip -- the `_host` twins of the device entry points (one twin per entry point).  A twin takes host
// pointers, checks its arguments, stages them through device buffers of its own, runs the device entry point on the null
// stream and copies the results back: the PCIe-inclusive path for callers without device memory of their own (small problems,
// tests, the torch-free command lines, the reference-side binding of INTEGRATION.md).  The twins hold no arithmetic; the
// kernels and their device entry points live in the other translation units.
#include <algorithm>
#include <vector>

#include "dig_genome2.hpp"
#include "dig_keyruns.hpp"
#include "dig_tiles.hpp"

using namespace dig;

namespace {

// The device side of one twin call.  The constructor selects the device; in() / out() / scratch() allocate a buffer the
// destructor frees (one byte at least, so an empty array still has an address) and in() copies its source up.  The first
// failing HIP call is recorded and the staging steps after it are skipped; staged() reports it (DIG_EHIP), and call() checks
// it before it runs the device entry point, then synchronises and copies every out() back.  Counts are elements of T; the
// _bytes forms serve run-time dtypes.
class Staging {
public:
    explicit Staging(int device) { check(hipSetDevice(device), "hipSetDevice"); }
    ~Staging()
    {
        for (void* p : bufs_) (void)hipFree(p);
    }
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;

    // a device copy of src[0, count); NULL for a NULL src (an optional input)
    template <typename T>
    const T* in(const T* src, size_t count)
    {
        return static_cast<const T*>(in_bytes(src, count * sizeof(T)));
    }
    // a device array of count elements that call() copies to dst
    template <typename T>
    T* out(T* dst, size_t count)
    {
        return static_cast<T*>(out_bytes(dst, count * sizeof(T)));
    }
    const void* in_bytes(const void* src, size_t bytes)
    {
        if (!src) return nullptr;
        void* d = alloc(bytes);
        if (d && bytes) check(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice), "hipMemcpy (host to device)");
        return d;
    }
    void* out_bytes(void* dst, size_t bytes)
    {
        void* d = alloc(bytes);
        outs_.push_back({dst, d, bytes});
        return d;
    }
    void* scratch(size_t bytes) { return alloc(bytes); }

    int staged() const
    {
        if (err_ != hipSuccess) return set_error(DIG_EHIP, "%s failed: %s", what_, hipGetErrorString(err_));
        return DIG_OK;
    }
    template <typename Fn, typename... Args>
    int call(Fn fn, Args... args)
    {
        if (int rc = staged()) return rc;
        if (int rc = fn(args...)) return rc;
        DIG_HIP_TRY(hipDeviceSynchronize());
        for (const Out& o : outs_)
            if (o.bytes) DIG_HIP_TRY(hipMemcpy(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost));
        return DIG_OK;
    }

private:
    struct Out {
        void* dst;
        const void* src;
        size_t bytes;
    };
    void* alloc(size_t bytes)
    {
        void* p = nullptr;
        if (err_ == hipSuccess && check(hipMalloc(&p, bytes ? bytes : 1), "hipMalloc")) bufs_.push_back(p);
        return p;
    }
    bool check(hipError_t e, const char* what)
    {
        if (e != hipSuccess && err_ == hipSuccess) err_ = e, what_ = what;
        return e == hipSuccess;
    }
    std::vector<void*> bufs_;
    std::vector<Out> outs_;
    hipError_t err_ = hipSuccess;
    const char* what_ = "";
};

using Nb3Fn = int (*)(const double*, const double*, const double*, double*, int64_t, void*);

int nb3_host(Nb3Fn fn, const double* k, const double* alpha, const double* p, double* out, int64_t n, int device)
{
    if (n == 0) return DIG_OK;
    if (!k || !alpha || !p || !out || n < 0) return set_error(DIG_EINVAL, "nb3_host: null pointer or negative n");
    Staging st(device);
    return st.call(fn, st.in(k, n), st.in(alpha, n), st.in(p, n), st.out(out, n), n, nullptr);
}

// the region table of the context-counting twins (`fn`: the twin's name, which the message begins with)
int check_regions(const char* fn, const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end, int64_t R, int n_chrom)
{
    for (int64_t r = 0; r < R; ++r) {
        DIG_REQUIRE_IN(fn, reg_chrom[r] >= 0 && reg_chrom[r] < n_chrom, "region chromosome index within [0, n_chrom)");
        DIG_REQUIRE_IN(fn, reg_start[r] >= 0 && reg_end[r] >= 0, "non-negative coordinates");
    }
    return DIG_OK;
}

// the cohorts' first global samples of the sorted-key twins
int check_sample_off(const char* fn, const int64_t* sample_off, int64_t C, int64_t n_samples)
{
    DIG_REQUIRE_IN(fn, sample_off[0] == 0 && sample_off[C] == n_samples, "sample_off: 0 first, the sample count last");
    for (int64_t c = 0; c < C; ++c) DIG_REQUIRE_IN(fn, sample_off[c] <= sample_off[c + 1], "sample_off non-decreasing");
    return DIG_OK;
}

int check_ascending(const char* fn, const int64_t* keys, int64_t n)
{
    for (int64_t i = 1; i < n; ++i) DIG_REQUIRE_IN(fn, keys[i - 1] <= keys[i], "keys ascending (the caller sorts)");
    return DIG_OK;
}

// st.call(fn, the ten genome arguments of H staged on the device, args...): the twins of the 2-bit genome's entry points
template <typename Fn, typename... Args>
int call_genome2(Staging& st, Fn fn, const Genome2& H, Args... args)
{
    const size_t nc = std::max(H.n_chrom, 1);
    return st.call(fn, st.in(H.words, H.n_words), H.n_words, st.in(H.nint_start, H.n_int), st.in(H.nint_end, H.n_int), H.n_int,
                   st.in(H.nint_bucket, H.n_int ? H.n_buckets : 0), H.n_buckets, st.in(H.chrom_off, nc), st.in(H.chrom_len, nc),
                   H.n_chrom, args...);
}

// What a twin that walks the 4-bit genome requires of the 14 arguments (check_tile_args) and, on its host arrays, of the genome
// and region tables: the checks no device entry point can make
int check_tile_tables_host(const char* fn, const TileArgs& a, bool dense)
{
    DIG_REQUIRE_IN(fn, a.n_up == 1 || a.n_up == 2, "n_up = n_down = 1 or 2");
    if (int rc = check_tile_args(fn, a, dense)) return rc;
    const TileGenome& g = a.g;
    static_assert(kCtxMaxPos == 16384, "the message below");
    for (int c = 0; c < (g.R ? g.n_chrom : 0); ++c)
        DIG_REQUIRE_IN(fn, g.chrom_off[c] >= 0 && g.chrom_len[c] >= 0 && (g.chrom_off[c] + g.chrom_len[c] + 7) / 8 + 1 <= g.n_words,
                       "chromosomes inside the genome array");
    for (int64_t r = 0; r < g.R; ++r) {
        DIG_REQUIRE_IN(fn, g.reg_chrom[r] >= 0 && g.reg_chrom[r] < g.n_chrom && g.reg_start[r] >= 0 && g.reg_end[r] >= 0,
                       "regions inside the genome table");
        DIG_REQUIRE_IN(fn, a.n_up == 1 || g.reg_end[r] - g.reg_start[r] <= kCtxMaxPos,
                       "a region of the general-context form holds at most 16 384 positions");
        DIG_REQUIRE_IN(fn, a.n_up == 1 || g.reg_start[r] == 0 || g.reg_start[r] >= a.n_up,
                       "a region that starts inside (0, n_up) would fetch from a negative position");
    }
    return DIG_OK;
}

// st.call(fn, the leading arguments of `a` up to C staged on the device, args...): the twins of the entry points that walk the 4-bit
// genome.  (The kernels load every cohort's table, whatever there is to write: a table that may be NULL then is staged as scratch.)
template <typename Fn, typename... Args>
int call_tile_genome(Staging& st, Fn fn, const TileArgs& a, Args... args)
{
    const TileGenome& g = a.g;
    const size_t nsp = (size_t)a.C * tile_contexts(a.n_up);
    const double* d_sp = a.s_prob ? st.in(a.s_prob, nsp) : static_cast<const double*>(st.scratch(nsp * sizeof(double)));
    return st.call(fn, st.in(g.words, g.n_words), g.n_words, st.in(g.chrom_off, g.n_chrom), st.in(g.chrom_len, g.n_chrom), g.n_chrom,
                   st.in(g.reg_chrom, g.R), st.in(g.reg_start, g.R), st.in(g.reg_end, g.R), g.R, d_sp, a.C, args...);
}

// the (mutation, region) pairs of the row-counting twins
int check_pairs_host(const char* fn, const int32_t* pair_mut, const int32_t* pair_reg, int64_t n_pairs, int64_t n_mut, int64_t R)
{
    for (int64_t i = 0; i < n_pairs; ++i)
        DIG_REQUIRE_IN(fn, pair_mut[i] >= 0 && pair_mut[i] < n_mut && pair_reg[i] >= 0 && pair_reg[i] < R,
                       "pairs inside the mutation / region tables");
    return DIG_OK;
}

// the gene table of the genic twins, once its pointers are known to be non-null
int check_gene_table(const char* fn, const int32_t* gene_chrom, const int64_t* blk_ptr, const int64_t* blk_start, const int64_t* blk_end,
                     const int64_t* cds_off, const int64_t* spl_ptr, const int64_t* spl_pos, int64_t n_genes, const int64_t* chrom_len,
                     int n_chrom)
{
    for (int64_t g = 0; g < n_genes; ++g) {
        DIG_REQUIRE_IN(fn, gene_chrom[g] >= 0 && gene_chrom[g] < n_chrom, "gene chromosome index within [0, n_chrom)");
        DIG_REQUIRE_IN(fn, blk_ptr[g] <= blk_ptr[g + 1] && spl_ptr[g] <= spl_ptr[g + 1], "blk_ptr, spl_ptr non-decreasing");
        int64_t len = 0;
        for (int64_t b = blk_ptr[g]; b < blk_ptr[g + 1]; ++b) {
            DIG_REQUIRE_IN(fn, blk_start[b] >= 1 && blk_start[b] <= blk_end[b] && blk_end[b] <= chrom_len[gene_chrom[g]],
                       "CDS blocks 1-based, closed, inside the chromosome");
            DIG_REQUIRE_IN(fn, b == blk_ptr[g] || blk_end[b - 1] < blk_start[b], "CDS blocks of a gene ascending and disjoint");
            DIG_REQUIRE_IN(fn, cds_off[b] == len, "cds_off: the CDS length in front of the block");
            len += blk_end[b] - blk_start[b] + 1;
        }
        DIG_REQUIRE_IN(fn, len % 3 == 0 && len <= INT32_MAX, "CDS length a multiple of 3 below 2^31");
        for (int64_t q = spl_ptr[g] + 1; q < spl_ptr[g + 1]; ++q) DIG_REQUIRE_IN(fn, spl_pos[q - 1] < spl_pos[q], "splice positions of a gene ascending");
    }
    return DIG_OK;
}

size_t dtype_size(int dt)
{
    switch (dt) {
        case DIG_F32: return 4;
        case DIG_F64: return 8;
        case DIG_I16: return 2;
        case DIG_BF16: return 2;
        default: return 0;
    }
}

// the tables of the two site-match twins: sites ascending with elements inside [0, E), rows inside their cohorts
int check_site_tables(const char* fn, const int64_t* site_pos, const int32_t* site_elt, int64_t S, int64_t E,
                      const int32_t* row_sample, const int32_t* row_cohort, const int64_t* sample_off, int64_t n, int64_t C,
                      int64_t n_samples)
{
    if (int rc = check_sample_off(fn, sample_off, C, n_samples)) return rc;
    for (int64_t j = 0; j < S; ++j) {
        DIG_REQUIRE_IN(fn, site_elt[j] >= 0 && site_elt[j] < E, "site element within [0, E)");
        DIG_REQUIRE_IN(fn, j == 0 || site_pos[j - 1] <= site_pos[j], "site_pos ascending (the caller sorts)");
    }
    for (int64_t i = 0; i < n; ++i) {
        DIG_REQUIRE_IN(fn, row_cohort[i] >= 0 && row_cohort[i] < C, "cohort within [0, C)");
        DIG_REQUIRE_IN(fn, row_sample[i] >= sample_off[row_cohort[i]] && row_sample[i] < sample_off[row_cohort[i] + 1],
                       "global sample within its cohort");
    }
    return DIG_OK;
}

}  // namespace

extern "C" {

int dig_nb_midp_upper_host(const double* k, const double* alpha, const double* p, double* out, int64_t n, int device)
{
    return nb3_host(dig_nb_midp_upper, k, alpha, p, out, n, device);
}
int dig_nb_exact_host(const double* k, const double* alpha, const double* p, double* out, int64_t n, int device)
{
    return nb3_host(dig_nb_exact, k, alpha, p, out, n, device);
}
int dig_nb_greater_host(const double* k, const double* alpha, const double* p, double* out, int64_t n, int device)
{
    return nb3_host(dig_nb_greater, k, alpha, p, out, n, device);
}
int dig_nb_midp_twosided_host(const double* k, const double* alpha, const double* p, double* out, int64_t n, int device)
{
    return nb3_host(dig_nb_midp_twosided, k, alpha, p, out, n, device);
}

int dig_fisher_host(const double* p1, const double* p2, double* out, int64_t n, int device)
{
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(p1 && p2 && out && n > 0, "non-null pointers, n >= 0");
    Staging st(device);
    return st.call(dig_fisher, st.in(p1, n), st.in(p2, n), st.out(out, n), n, nullptr);
}

int dig_normal_params_to_gamma_host(const double* mu, const double* sigma, double* alpha, double* theta, int64_t n, int device)
{
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(mu && sigma && alpha && theta && n > 0, "non-null pointers, n >= 0");
    Staging st(device);
    return st.call(dig_normal_params_to_gamma, st.in(mu, n), st.in(sigma, n), st.out(alpha, n), st.out(theta, n), n, nullptr);
}

int dig_element_stats_host(const double* mu, const double* sigma, const double* mu_indel, const double* sigma_indel,
                           const double* pi_sum, const double* pi_indel, int pi_indel_per_cohort, const int32_t* obs_snv,
                           const int32_t* obs_samples, const int32_t* obs_indel, const double* cj, const double* cj_indel, double* out,
                           int64_t E, int64_t C, int device)
{
    DIG_REQUIRE(E >= 0 && C >= 0, "E, C >= 0");
    if (E == 0 || C == 0) return DIG_OK;
    DIG_REQUIRE(mu && sigma && pi_sum && pi_indel && obs_snv && obs_samples && obs_indel && cj && cj_indel && out,
                "non-null pointers");
    DIG_REQUIRE(!mu_indel || sigma_indel, "sigma_indel with mu_indel");
    const size_t n = (size_t)E * C;
    const int64_t wsb = dig_element_stats_workspace(E, C);
    Staging st(device);
    return st.call(dig_element_stats, st.in(mu, n), st.in(sigma, n), st.in(mu_indel, n), mu_indel ? st.in(sigma_indel, n) : nullptr,
                   st.in(pi_sum, n), st.in(pi_indel, pi_indel_per_cohort ? n : (size_t)E), pi_indel_per_cohort, st.in(obs_snv, n),
                   st.in(obs_samples, n), st.in(obs_indel, n), st.in(cj, C), st.in(cj_indel, C), st.out(out, n * DIG_ES_NPLANES),
                   E, C, wsb > 0 ? st.scratch((size_t)wsb) : nullptr, wsb, nullptr);
}

int dig_tiled_nb_test_host(const double* pt, int pt_per_cohort, const int32_t* k, const double* mu, const double* sigma,
                           double* pval, double* exp_out, int64_t C, int64_t n_bins, int64_t n_tiles, int device)
{
    DIG_REQUIRE(C >= 0 && n_bins >= 0 && n_tiles >= 0, "non-negative sizes");
    const size_t n = (size_t)C * n_bins * n_tiles;
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(pt && k && mu && sigma && pval && exp_out, "non-null pointers");
    const size_t ncb = (size_t)C * n_bins;
    Staging st(device);
    return st.call(dig_tiled_nb_test, st.in(pt, pt_per_cohort ? n : (size_t)n_bins * n_tiles), pt_per_cohort, st.in(k, n),
                   st.in(mu, ncb), st.in(sigma, ncb), st.out(pval, n), st.out(exp_out, n), C, n_bins, n_tiles, nullptr);
}

int dig_accumulate_elements_host(const double* bin_mu, const double* bin_std, const int32_t* bin_y, const uint8_t* bin_flag,
                                 const int32_t* bin_ctx, const int64_t* ov_ptr, const int32_t* ov_idx, const int32_t* L, int n_class,
                                 const uint8_t* strand_minus, const int32_t* gene_length, const double* d_pr, double* MU,
                                 double* SIGMA, int32_t* R_OBS, int32_t* FLAG, double* P, int32_t* R_SIZE, int32_t* ELT_SIZE,
                                 double* P_INDEL, int64_t N, int64_t E, int64_t C, int device)
{
    DIG_REQUIRE(N >= 0 && E >= 0 && C >= 0, "N, E, C >= 0");
    DIG_REQUIRE(n_class == 1 || n_class == 4, "n_class must be 1 (elements) or 4 (genes)");
    if (E == 0 || C == 0) return DIG_OK;
    DIG_REQUIRE(bin_mu && bin_std && bin_y && bin_flag && bin_ctx && ov_ptr && ov_idx && L && strand_minus && d_pr,
                "non-null inputs");
    DIG_REQUIRE(MU && SIGMA && R_OBS && FLAG && P && R_SIZE && ELT_SIZE && P_INDEL, "non-null outputs");
    const int64_t nnz = ov_ptr[E];
    DIG_REQUIRE(nnz >= 0, "ov_ptr[E] >= 0");
    for (int64_t q = 0; q < nnz; ++q) DIG_REQUIRE(ov_idx[q] >= 0 && ov_idx[q] < N, "ov_idx within [0, N)");
    const size_t nNC = (size_t)N * C, nEC = (size_t)E * C;
    const int64_t wsb = dig_accumulate_workspace(E, C);
    Staging st(device);
    return st.call(dig_accumulate_elements, st.in(bin_mu, nNC), st.in(bin_std, nNC), st.in(bin_y, nNC), st.in(bin_flag, nNC),
                   st.in(bin_ctx, (size_t)N * 64), st.in(ov_ptr, (size_t)E + 1), st.in(ov_idx, (size_t)nnz),
                   st.in(L, (size_t)E * n_class * 192), n_class, st.in(strand_minus, E), st.in(gene_length, E),
                   st.in(d_pr, (size_t)C * 192), st.out(MU, nEC), st.out(SIGMA, nEC), st.out(R_OBS, nEC), st.out(FLAG, nEC),
                   st.out(P, nEC * n_class), st.out(R_SIZE, E), st.out(ELT_SIZE, E), st.out(P_INDEL, E), N, E, C,
                   st.scratch((size_t)wsb), wsb, nullptr);
}

int dig_gene_stats_host(const double* mu, const double* sigma, const double* mu_indel, const double* sigma_indel, const double* pi,
                        int n_pi, const double* pi_indel, int pi_indel_per_cohort, const int32_t* obs, const int32_t* n_samp,
                        const double* cj, const double* t_indel, int with_indel, double* out, int64_t G, int64_t C, int device)
{
    DIG_REQUIRE(G >= 0 && C >= 0, "G, C >= 0");
    DIG_REQUIRE(n_pi == 4 || n_pi == 6, "n_pi: 4 or 6");
    if (G == 0 || C == 0) return DIG_OK;
    DIG_REQUIRE(mu && sigma && pi && obs && n_samp && cj && out, "non-null pointers");
    DIG_REQUIRE(!with_indel || (pi_indel && t_indel), "pi_indel and t_indel for the indel block");
    const size_t nGC = (size_t)G * C;
    Staging st(device);
    return st.call(dig_gene_stats, st.in(mu, nGC), st.in(sigma, nGC), st.in(mu_indel, nGC), st.in(sigma_indel, nGC),
                   st.in(pi, nGC * n_pi), n_pi, st.in(pi_indel, pi_indel_per_cohort ? nGC : (size_t)G), pi_indel_per_cohort,
                   st.in(obs, nGC * 5), st.in(n_samp, nGC * 6), st.in(cj, C), st.in(t_indel, C), with_indel, st.out(out, nGC * 22),
                   G, C, nullptr);
}

int dig_gene_selection_host(const double* alpha, const double* theta, const double* pi, int n_pi, const int32_t* obs, double* out,
                            int64_t G, int64_t C, int device)
{
    DIG_REQUIRE(G >= 0 && C >= 0, "G, C >= 0");
    DIG_REQUIRE(n_pi == 4 || n_pi == 6, "n_pi: 4 or 6");
    if (G == 0 || C == 0) return DIG_OK;
    DIG_REQUIRE(alpha && theta && pi && obs && out, "non-null pointers");
    const size_t nGC = (size_t)G * C;
    Staging st(device);
    return st.call(dig_gene_selection, st.in(alpha, nGC), st.in(theta, nGC), st.in(pi, nGC * n_pi), n_pi, st.in(obs, nGC * 5),
                   st.out(out, nGC * DIG_SEL_NPLANES), G, C, nullptr);
}

int dig_gene_row_keys_host(const int32_t* gene, const int32_t* sample, const uint8_t* annot, const int32_t* cohort,
                           const int64_t* sample_off, int64_t n, int64_t G, int64_t C, int64_t n_samples, int64_t* keys,
                           int32_t* sample_total, int device)
{
    DIG_REQUIRE(n >= 0 && G >= 0 && C >= 1 && n_samples >= 0, "n, G, n_samples >= 0, C >= 1");
    DIG_REQUIRE(sample_off && (n == 0 || (gene && sample && annot && cohort && keys)) && (n_samples == 0 || sample_total),
                "non-null pointers");
    int sb = 0;
    if (int rc = gene_key_layout(__func__, G, C, n_samples, &sb)) return rc;
    if (int rc = check_sample_off(__func__, sample_off, C, n_samples)) return rc;
    for (int64_t i = 0; i < n; ++i) {
        DIG_REQUIRE(cohort[i] >= 0 && cohort[i] < C, "cohort within [0, C)");
        DIG_REQUIRE(gene[i] >= 0 && gene[i] <= G + 1, "gene id within [0, G + 1]");
        DIG_REQUIRE(annot[i] <= 5, "annotation class within [0, 5]");
        DIG_REQUIRE(sample[i] >= 0 && sample_off[cohort[i]] + sample[i] < sample_off[cohort[i] + 1], "sample id within its cohort");
    }
    Staging st(device);
    return st.call(dig_gene_row_keys, st.in(gene, n), st.in(sample, n), st.in(annot, n), st.in(cohort, n), st.in(sample_off, C + 1), n,
                   G, C, n_samples, st.out(keys, n), st.out(sample_total, n_samples), nullptr);
}

int dig_gene_counts_host(const int64_t* keys_sorted, int64_t n, const int32_t* sample_total, int64_t n_samples,
                         double max_muts_per_sample, double max_muts_per_gene_per_sample, int64_t tp53, int64_t G, int64_t C,
                         int32_t* obs, int32_t* n_samp, int32_t* extra, int64_t* n_syn, uint8_t* blacklisted, int device)
{
    DIG_REQUIRE(n >= 0 && G >= 0 && C >= 1 && n_samples >= 0, "n, G, n_samples >= 0, C >= 1");
    DIG_REQUIRE(n_syn && (n == 0 || keys_sorted) && (G == 0 || (obs && n_samp && extra)) && (n_samples == 0 || (sample_total && blacklisted)),
                "non-null pointers");
    int sb = 0;
    if (int rc = gene_key_layout(__func__, G, C, n_samples, &sb)) return rc;
    if (int rc = check_ascending(__func__, keys_sorted, n)) return rc;
    const size_t GC = (size_t)G * C;
    Staging st(device);
    return st.call(dig_gene_counts, st.in(keys_sorted, n), n, st.in(sample_total, n_samples), n_samples, max_muts_per_sample,
                   max_muts_per_gene_per_sample, tp53, G, C, st.out(obs, GC * 5), st.out(n_samp, GC * 6), st.out(extra, GC * 2),
                   st.out(n_syn, C), st.out(blacklisted, n_samples), static_cast<int32_t*>(st.scratch(GC * 5 * sizeof(int32_t))), nullptr);
}

int dig_panel_row_keys_host(const int32_t* label, const int32_t* sample, const uint8_t* annot, const int32_t* cohort,
                            const int64_t* sample_off, const uint8_t* skip, const uint32_t* label_mask, int64_t n, int64_t L, int64_t P,
                            int64_t C, int64_t n_samples, int64_t* keys, int64_t* n_cds, int device)
{
    DIG_REQUIRE(n >= 0, "n >= 0");
    int lb = 0;
    if (int rc = panel_key_layout(__func__, L, P, C, n_samples, &lb)) return rc;
    DIG_REQUIRE(sample_off && label_mask && n_cds && (n == 0 || (label && sample && annot && cohort && keys)), "non-null pointers");
    if (int rc = check_sample_off(__func__, sample_off, C, n_samples)) return rc;
    for (int64_t i = 0; i < n; ++i) {
        DIG_REQUIRE(cohort[i] >= 0 && cohort[i] < C, "cohort within [0, C)");
        DIG_REQUIRE(label[i] >= 0 && label[i] <= L, "label within [0, L]");
        DIG_REQUIRE(annot[i] <= 6, "annotation class within [0, 6]");
        DIG_REQUIRE(sample[i] >= 0 && sample_off[cohort[i]] + sample[i] < sample_off[cohort[i] + 1], "sample id within its cohort");
    }
    Staging st(device);
    return st.call(dig_panel_row_keys, st.in(label, n), st.in(sample, n), st.in(annot, n), st.in(cohort, n), st.in(sample_off, C + 1),
                   st.in(skip, n_samples), st.in(label_mask, L), n, L, P, C, n_samples, st.out(keys, n), st.out(n_cds, C), nullptr);
}

int dig_panel_counts_host(const int64_t* keys_sorted, int64_t n, const uint32_t* label_mask, const int64_t* sample_off, int64_t L,
                          int64_t P, int64_t C, int64_t n_samples, int64_t* n_mut, int64_t* n_pairs, int64_t* n_sample, int device)
{
    DIG_REQUIRE(n >= 0, "n >= 0");
    int lb = 0;
    if (int rc = panel_key_layout(__func__, L, P, C, n_samples, &lb)) return rc;
    DIG_REQUIRE(sample_off && label_mask && n_mut && n_pairs && n_sample && (n == 0 || keys_sorted), "non-null pointers");
    if (int rc = check_sample_off(__func__, sample_off, C, n_samples)) return rc;
    if (int rc = check_ascending(__func__, keys_sorted, n)) return rc;
    const size_t CP = (size_t)C * P;
    Staging st(device);
    return st.call(dig_panel_counts, st.in(keys_sorted, n), n, st.in(label_mask, L), st.in(sample_off, C + 1), L, P, C, n_samples,
                   st.out(n_mut, CP), st.out(n_pairs, CP), st.out(n_sample, CP), nullptr);
}

int dig_window_pair_keys_host(const int32_t* pair_row, const int32_t* pair_blk, int64_t n_pairs, const int32_t* blk_window, int64_t n_blk,
                              const int32_t* row_sample, const int32_t* row_uid, const uint8_t* row_indel, int64_t n_rows,
                              int64_t n_samples, int64_t N, int64_t n_uid, int64_t* keys, int device)
{
    DIG_REQUIRE(n_pairs >= 0 && n_blk >= 0 && n_rows >= 0, "n_pairs, n_blk, n_rows >= 0");
    WindowKeyLayout lay;
    if (int rc = window_key_layout(__func__, n_samples, N, n_uid, &lay)) return rc;
    DIG_REQUIRE(n_pairs == 0 || (pair_row && pair_blk && keys), "non-null pair arrays");
    DIG_REQUIRE(n_rows == 0 || (row_sample && row_uid && row_indel), "non-null row arrays");
    for (int64_t b = 0; blk_window && b < n_blk; ++b) DIG_REQUIRE(blk_window[b] >= 0 && blk_window[b] < N, "window within [0, N)");
    DIG_REQUIRE(blk_window || n_blk <= N, "without blk_window the block row is the window: n_blk <= N");
    for (int64_t r = 0; r < n_rows; ++r) {
        DIG_REQUIRE(row_sample[r] >= 0 && row_sample[r] < n_samples, "global sample within [0, n_samples)");
        DIG_REQUIRE(row_uid[r] >= 0 && row_uid[r] < n_uid, "mutation id within [0, n_uid)");
    }
    for (int64_t i = 0; i < n_pairs; ++i)
        DIG_REQUIRE(pair_row[i] >= 0 && pair_row[i] < n_rows && pair_blk[i] >= 0 && pair_blk[i] < n_blk, "a pair within the tables");
    Staging st(device);
    return st.call(dig_window_pair_keys, st.in(pair_row, n_pairs), st.in(pair_blk, n_pairs), n_pairs, st.in(blk_window, n_blk), n_blk,
                   st.in(row_sample, n_rows), st.in(row_uid, n_rows), st.in(row_indel, n_rows), n_rows, n_samples, N, n_uid,
                   st.out(keys, n_pairs), nullptr);
}

int dig_window_sample_hits_host(const int64_t* keys_sorted, int64_t n_pairs, int64_t n_samples, int64_t N, int64_t n_uid, int32_t* hits,
                                int device)
{
    DIG_REQUIRE(n_pairs >= 0, "n_pairs >= 0");
    WindowKeyLayout lay;
    if (int rc = window_key_layout(__func__, n_samples, N, n_uid, &lay)) return rc;
    DIG_REQUIRE((n_pairs == 0 || keys_sorted) && (n_samples == 0 || hits), "non-null pointers");
    if (int rc = check_ascending(__func__, keys_sorted, n_pairs)) return rc;
    Staging st(device);
    return st.call(dig_window_sample_hits, st.in(keys_sorted, n_pairs), n_pairs, n_samples, N, n_uid, st.out(hits, n_samples), nullptr);
}

int dig_window_objectives_host(const int64_t* keys_sorted, int64_t n_pairs, const uint8_t* keep, const int64_t* sample_off,
                               int64_t n_samples, int64_t N, int64_t C, int64_t n_uid, double* labels, int device)
{
    DIG_REQUIRE(n_pairs >= 0 && C >= 1, "n_pairs >= 0, C >= 1");
    WindowKeyLayout lay;
    if (int rc = window_key_layout(__func__, n_samples, N, n_uid, &lay)) return rc;
    DIG_REQUIRE(N < ((int64_t)1 << 62) / C, "N C below 2^62");
    DIG_REQUIRE(sample_off && (n_pairs == 0 || keys_sorted) && (n_samples == 0 || keep) && (N == 0 || labels), "non-null pointers");
    if (int rc = check_sample_off(__func__, sample_off, C, n_samples)) return rc;
    if (int rc = check_ascending(__func__, keys_sorted, n_pairs)) return rc;
    const size_t NC = (size_t)N * C;
    Staging st(device);
    return st.call(dig_window_objectives, st.in(keys_sorted, n_pairs), n_pairs, st.in(keep, n_samples), st.in(sample_off, C + 1), n_samples,
                   N, C, n_uid, st.out(labels, NC), static_cast<int32_t*>(st.scratch(NC * sizeof(int32_t))), nullptr);
}

int dig_cnv_segment_deltas_host(const int64_t* win_start, const int64_t* chrom_id, const int64_t* chrom_off, int64_t n_chrom, int64_t N,
                                int64_t W, const int64_t* seg_chrom, const int64_t* seg_start, const int64_t* seg_end,
                                const uint8_t* seg_class, const int32_t* seg_weight, const int32_t* seg_cohort, int64_t n_seg, int64_t C,
                                int64_t* deltas, int device)
{
    DIG_REQUIRE(n_chrom >= 0 && n_chrom <= N && n_seg >= 0, "0 <= n_chrom <= N, n_seg >= 0");
    CnvSizes sz;
    if (int rc = cnv_sizes(__func__, C, N, W, &sz)) return rc;
    DIG_REQUIRE(deltas && chrom_off && (N == 0 || (win_start && chrom_id)), "non-null window tables and deltas");
    DIG_REQUIRE(n_seg == 0 || (seg_chrom && seg_start && seg_end && seg_class && seg_weight && seg_cohort), "non-null segment arrays");
    DIG_REQUIRE(chrom_off[0] == 0 && chrom_off[n_chrom] == N, "chrom_off: 0 first, N last");
    for (int64_t r = 0; r < n_chrom; ++r) {
        DIG_REQUIRE(chrom_off[r] < chrom_off[r + 1], "chrom_off ascending: every chromosome of chrom_id has a window");
        DIG_REQUIRE(r == 0 || chrom_id[r - 1] < chrom_id[r], "chrom_id ascending");
        for (int64_t n = chrom_off[r]; n < chrom_off[r + 1]; ++n) {
            DIG_REQUIRE(win_start[n] >= 0 && win_start[n] < ((int64_t)1 << 40), "window starts within [0, 2^40)");
            DIG_REQUIRE(n == chrom_off[r] || win_start[n - 1] < win_start[n], "window starts distinct and ascending within a chromosome");
        }
    }
    for (int64_t i = 0; i < n_seg; ++i) {
        DIG_REQUIRE(seg_start[i] >= 0 && seg_start[i] < seg_end[i] && seg_end[i] <= ((int64_t)1 << 40), "segments with 0 <= start < end <= 2^40");
        DIG_REQUIRE(seg_class[i] <= 2 && seg_weight[i] >= 1, "class within [0, 2], weight >= 1");
        DIG_REQUIRE(seg_cohort[i] >= 0 && seg_cohort[i] < C, "cohort within [0, C)");
    }
    Staging st(device);
    return st.call(dig_cnv_segment_deltas, st.in(win_start, N), st.in(chrom_id, n_chrom), st.in(chrom_off, n_chrom + 1), n_chrom, N, W,
                   st.in(seg_chrom, n_seg), st.in(seg_start, n_seg), st.in(seg_end, n_seg), st.in(seg_class, n_seg), st.in(seg_weight, n_seg),
                   st.in(seg_cohort, n_seg), n_seg, C, st.out(deltas, (size_t)sz.delta_bytes / sizeof(int64_t)), nullptr);
}

int dig_cnv_window_means_host(const int64_t* deltas, int64_t N, int64_t C, int64_t W, double* labels, int device)
{
    CnvSizes sz;
    if (int rc = cnv_sizes(__func__, C, N, W, &sz)) return rc;
    if (N == 0) return DIG_OK;
    DIG_REQUIRE(deltas && labels, "non-null pointers");
    Staging st(device);
    return st.call(dig_cnv_window_means, st.in(deltas, (size_t)sz.delta_bytes / sizeof(int64_t)), N, C, W, st.out(labels, (size_t)C * N * 3),
                   static_cast<int64_t*>(st.scratch((size_t)sz.carry_bytes)), nullptr);
}

int dig_sequence_counts_host(const int32_t* pair_row, int64_t n_pairs, const int32_t* row_type, const int32_t* row_cohort, int64_t n,
                             int64_t K, int64_t C, int64_t* counts, int device)
{
    DIG_REQUIRE(n_pairs >= 0 && n >= 0, "n_pairs, n >= 0");
    DIG_REQUIRE(K >= 1 && K <= kSeqMaxK, "K within [1, 3072] (the workgroup's LDS counters)");
    DIG_REQUIRE(C >= 1 && C < ((int64_t)1 << 31), "C within [1, 2^31)");
    DIG_REQUIRE(counts && (n == 0 || (row_type && row_cohort)) && (n_pairs == 0 || pair_row), "non-null pointers");
    for (int64_t r = 0; r < n; ++r) {
        DIG_REQUIRE(row_cohort[r] >= 0 && row_cohort[r] < C, "cohort within [0, C)");
        DIG_REQUIRE(row_type[r] >= 0 && row_type[r] <= K, "type within [0, K] (K: no table entry)");
    }
    for (int64_t i = 0; i < n_pairs; ++i) DIG_REQUIRE(pair_row[i] >= 0 && pair_row[i] < n, "a pair within the rows");
    Staging st(device);
    return st.call(dig_sequence_counts, st.in(pair_row, n_pairs), n_pairs, st.in(row_type, n), st.in(row_cohort, n), n, K, C,
                   st.out(counts, (size_t)C * K), nullptr);
}

int dig_site_match_count_host(const int64_t* site_pos, const int64_t* site_end, const int64_t* site_attr, const int32_t* site_elt,
                              int64_t S, int64_t E, const int64_t* row_pos, const int64_t* row_end, const int64_t* row_attr,
                              const int32_t* row_sample, const int32_t* row_cohort, const int64_t* sample_off, int64_t n, int64_t C,
                              int64_t n_samples, int32_t* counts, int device)
{
    DIG_REQUIRE(S >= 0 && S < ((int64_t)1 << 31) && n >= 0, "0 <= S < 2^31, n >= 0");
    int sb = 0;
    if (int rc = site_key_layout(__func__, E, C, n_samples, &sb)) return rc;
    DIG_REQUIRE(sample_off && (S == 0 || (site_pos && site_end && site_attr && site_elt)), "non-null sample_off, site arrays");
    DIG_REQUIRE(n == 0 || (row_pos && row_end && row_attr && row_sample && row_cohort && counts), "non-null row arrays, counts");
    if (int rc = check_site_tables(__func__, site_pos, site_elt, S, E, row_sample, row_cohort, sample_off, n, C, n_samples))
        return rc;
    Staging st(device);
    return st.call(dig_site_match_count, st.in(site_pos, S), st.in(site_end, S), st.in(site_attr, S), st.in(site_elt, S), S, E,
                   st.in(row_pos, n), st.in(row_end, n), st.in(row_attr, n), st.in(row_sample, n), st.in(row_cohort, n),
                   st.in(sample_off, C + 1), n, C, n_samples, st.out(counts, n), nullptr);
}

int dig_site_match_keys_host(const int64_t* site_pos, const int64_t* site_end, const int64_t* site_attr, const int32_t* site_elt,
                             int64_t S, int64_t E, const int64_t* row_pos, const int64_t* row_end, const int64_t* row_attr,
                             const int32_t* row_sample, const int32_t* row_cohort, const int64_t* sample_off, int64_t n, int64_t C,
                             int64_t n_samples, const int64_t* offsets, int64_t total, int64_t* keys, int device)
{
    DIG_REQUIRE(S >= 0 && S < ((int64_t)1 << 31) && n >= 0 && total >= 0, "0 <= S < 2^31, n, total >= 0");
    int sb = 0;
    if (int rc = site_key_layout(__func__, E, C, n_samples, &sb)) return rc;
    DIG_REQUIRE(sample_off && (S == 0 || (site_pos && site_end && site_attr && site_elt)), "non-null sample_off, site arrays");
    DIG_REQUIRE(n == 0 || (row_pos && row_end && row_attr && row_sample && row_cohort && offsets), "non-null row arrays, offsets");
    DIG_REQUIRE(total == 0 || keys, "non-null keys");
    if (int rc = check_site_tables(__func__, site_pos, site_elt, S, E, row_sample, row_cohort, sample_off, n, C, n_samples))
        return rc;
    for (int64_t i = 0; i < n; ++i)
        DIG_REQUIRE(offsets[i] >= (i ? offsets[i - 1] : 0) && offsets[i] <= total, "offsets: an exclusive prefix sum, 0 first, within total");
    Staging st(device);
    return st.call(dig_site_match_keys, st.in(site_pos, S), st.in(site_end, S), st.in(site_attr, S), st.in(site_elt, S), S, E,
                   st.in(row_pos, n), st.in(row_end, n), st.in(row_attr, n), st.in(row_sample, n), st.in(row_cohort, n),
                   st.in(sample_off, C + 1), n, C, n_samples, st.in(offsets, n), total, st.out(keys, total), nullptr);
}

int dig_site_counts_host(const int64_t* keys_sorted, int64_t total, int64_t E, int64_t C, int64_t n_samples, int32_t* obs_snv,
                         int32_t* obs_samples, int device)
{
    DIG_REQUIRE(total >= 0, "total >= 0");
    int sb = 0;
    if (int rc = site_key_layout(__func__, E, C, n_samples, &sb)) return rc;
    DIG_REQUIRE((total == 0 || keys_sorted) && (E == 0 || (obs_snv && obs_samples)), "non-null pointers");
    if (int rc = check_ascending(__func__, keys_sorted, total)) return rc;
    const size_t EC = (size_t)E * C;
    Staging st(device);
    return st.call(dig_site_counts, st.in(keys_sorted, total), total, E, C, n_samples, st.out(obs_snv, EC), st.out(obs_samples, EC),
                   nullptr);
}

int dig_tile_select_count_host(const double* score, const int32_t* n_valid, const double* cut, int64_t C, int64_t R, int64_t T,
                               int32_t* counts, int device)
{
    if (int rc = tile_select_sizes(__func__, C, R, T)) return rc;
    const size_t rows = (size_t)C * R;
    if (rows == 0) return DIG_OK;
    DIG_REQUIRE(counts && (T == 0 || (score && n_valid && cut)), "non-null score, n_valid, cut, counts");
    Staging st(device);
    return st.call(dig_tile_select_count, st.in(score, rows * T), st.in(n_valid, R), st.in(cut, C), C, R, T, st.out(counts, rows),
                   nullptr);
}

int dig_tile_select_fill_host(const double* score, const int32_t* n_valid, const double* cut, int64_t C, int64_t R, int64_t T,
                              const int64_t* offsets, int64_t total, const double* pt, const double* exp_in, const int32_t* k,
                              int32_t* hit_region, int32_t* hit_tile, double* hit_score, double* hit_pt, double* hit_exp,
                              int32_t* hit_k, int device)
{
    if (int rc = tile_select_sizes(__func__, C, R, T)) return rc;
    DIG_REQUIRE(total >= 0, "total >= 0");
    const size_t rows = (size_t)C * R, n = rows * T;
    if (n == 0 || total == 0) return DIG_OK;
    DIG_REQUIRE(score && n_valid && cut && offsets, "non-null score, n_valid, cut, offsets");
    for (size_t i = 0; i < rows; ++i)
        DIG_REQUIRE(offsets[i] >= (i ? offsets[i - 1] : 0) && offsets[i] <= total, "offsets: an exclusive prefix sum, 0 first, within total");
    Staging st(device);
    // (an output the call skips -- NULL, or without its plane -- is not staged: the caller's array stays as it was)
    const size_t nt = (size_t)total;
    return st.call(dig_tile_select_fill, st.in(score, n), st.in(n_valid, R), st.in(cut, C), C, R, T, st.in(offsets, rows), total,
                   st.in(pt, n), st.in(exp_in, n), st.in(k, n), hit_region ? st.out(hit_region, nt) : nullptr,
                   hit_tile ? st.out(hit_tile, nt) : nullptr, hit_score ? st.out(hit_score, nt) : nullptr,
                   hit_pt && pt ? st.out(hit_pt, nt) : nullptr, hit_exp && exp_in ? st.out(hit_exp, nt) : nullptr,
                   hit_k && k ? st.out(hit_k, nt) : nullptr, nullptr);
}

// the offsets of a row-select twin: an exclusive prefix sum within total
static int check_row_offsets(const char* fn, const int64_t* offsets, size_t n, int64_t total)
{
    for (size_t i = 0; i < n; ++i)
        DIG_REQUIRE_IN(fn, offsets[i] >= (i ? offsets[i - 1] : 0) && offsets[i] <= total,
                       "offsets: an exclusive prefix sum, 0 first, within total");
    return DIG_OK;
}

int dig_row_select_count_host(const double* score, const double* cut, int64_t rows, int64_t n, int32_t* counts, int device)
{
    int64_t chunks = 0;
    if (int rc = row_select_sizes(__func__, rows, n, &chunks)) return rc;
    const size_t slots = (size_t)rows * chunks;
    if (slots == 0) return DIG_OK;
    DIG_REQUIRE(score && cut && counts, "non-null score, cut, counts");
    Staging st(device);
    return st.call(dig_row_select_count, st.in(score, (size_t)rows * n), st.in(cut, rows), rows, n, st.out(counts, slots), nullptr);
}

int dig_row_select_fill_host(const double* score, const double* cut, int64_t rows, int64_t n, const int64_t* offsets, int64_t total,
                             int32_t* hit_index, double* hit_score, int device)
{
    int64_t chunks = 0;
    if (int rc = row_select_sizes(__func__, rows, n, &chunks)) return rc;
    DIG_REQUIRE(total >= 0, "total >= 0");
    const size_t slots = (size_t)rows * chunks;
    if (slots == 0 || total == 0) return DIG_OK;
    DIG_REQUIRE(score && cut && offsets, "non-null score, cut, offsets");
    if (int rc = check_row_offsets(__func__, offsets, slots, total)) return rc;
    Staging st(device);
    // (an output the call skips is not staged: the caller's array stays as it was)
    return st.call(dig_row_select_fill, st.in(score, (size_t)rows * n), st.in(cut, rows), rows, n, st.in(offsets, slots), total,
                   hit_index ? st.out(hit_index, (size_t)total) : nullptr, hit_score ? st.out(hit_score, (size_t)total) : nullptr,
                   nullptr);
}

int dig_row_scatter_host(const double* score, const double* cut, int64_t rows, int64_t n, const int64_t* offsets, int64_t total,
                         const double* values, double fill, double* out, int device)
{
    int64_t chunks = 0;
    if (int rc = row_select_sizes(__func__, rows, n, &chunks)) return rc;
    DIG_REQUIRE(total >= 0, "total >= 0");
    const size_t slots = (size_t)rows * chunks;
    if (slots == 0) return DIG_OK;
    DIG_REQUIRE(score && cut && offsets && out && (values || total == 0), "non-null score, cut, offsets, out, values");
    if (int rc = check_row_offsets(__func__, offsets, slots, total)) return rc;
    Staging st(device);
    return st.call(dig_row_scatter, st.in(score, (size_t)rows * n), st.in(cut, rows), rows, n, st.in(offsets, slots), total,
                   st.in(values, (size_t)total), fill, st.out(out, (size_t)rows * n), nullptr);
}

int dig_group_fisher_host(const double* p, const uint8_t* member, int64_t R, int64_t C, int64_t E, int64_t M, double* out_p, int32_t* out_n,
                          int device)
{
    int64_t chunks = 0;
    if (int rc = group_sizes(__func__, R, C, E, M, &chunks)) return rc;
    const size_t n_out = (size_t)R * M * E, n_in = (size_t)R * C * E;
    if (n_out == 0) return DIG_OK;
    DIG_REQUIRE(out_p && (C == 0 || (p && member)), "non-null p, member, out_p");
    Staging st(device);
    return st.call(dig_group_fisher, st.in(p, n_in), st.in(member, (size_t)M * C), R, C, E, M, st.out(out_p, n_out),
                   out_n ? st.out(out_n, n_out) : nullptr, nullptr);
}

int dig_group_sums_host(const double* x, const double* gate, const uint8_t* member, int64_t R, int64_t C, int64_t E, int64_t M, double* out,
                        int device)
{
    int64_t chunks = 0;
    if (int rc = group_sizes(__func__, R, C, E, M, &chunks)) return rc;
    const size_t n_out = (size_t)R * M * E, n_in = (size_t)R * C * E;
    if (n_out == 0) return DIG_OK;
    DIG_REQUIRE(out && (C == 0 || (x && member)), "non-null x, member, out");
    Staging st(device);
    return st.call(dig_group_sums, st.in(x, n_in), st.in(gate, n_in), st.in(member, (size_t)M * C), R, C, E, M, st.out(out, n_out),
                   nullptr);
}

int dig_nb_power_host(const double* alpha, const double* theta, const double* pi, const double* scale, const double* level, int64_t rows,
                      int64_t n, const double* folds, int n_folds, int32_t k_max, int32_t* k_crit, double* power, int device)
{
    int64_t chunks = 0;
    if (int rc = nb_power_sizes(__func__, rows, n, folds, n_folds, k_max, power, &chunks)) return rc;
    for (int j = 0; j < n_folds; ++j) DIG_REQUIRE(folds[j] > 0.0 && folds[j] < HUGE_VAL, "folds finite and > 0");
    const size_t m = (size_t)rows * n;
    if (m == 0) return DIG_OK;
    DIG_REQUIRE(alpha && theta && pi && level && k_crit, "non-null alpha, theta, pi, level, k_crit");
    Staging st(device);
    return st.call(dig_nb_power, st.in(alpha, m), st.in(theta, m), st.in(pi, m), st.in(scale, rows), st.in(level, rows), rows, n,
                   st.in(folds, n_folds), n_folds, k_max, st.out(k_crit, m), n_folds ? st.out(power, m * n_folds) : nullptr, nullptr);
}

int dig_map_windows_host(const double* mu_cm, const double* std_cm, const int32_t* y_cm, const uint8_t* flag_cm, int64_t C, int64_t N,
                         const int64_t* run_ptr, int64_t M, int drop_flagged, int tail, int32_t* n_bins, int64_t* y_true, double* y_pred,
                         double* std, double* pval, int device)
{
    MapWindowPlan plan{};
    if (int rc = map_windows_sizes(__func__, C, N, M, drop_flagged, tail, flag_cm, &plan)) return rc;
    if (C * M == 0) return DIG_OK;
    DIG_REQUIRE(run_ptr && n_bins && y_true && y_pred && std && pval, "non-null run_ptr, n_bins, y_true, y_pred, std, pval");
    DIG_REQUIRE(N == 0 || (mu_cm && std_cm && y_cm), "non-null mu_cm, std_cm, y_cm");
    DIG_REQUIRE(run_ptr[0] >= 0 && run_ptr[M] == N, "run_ptr: non-negative first, N last");
    for (int64_t m = 0; m < M; ++m) DIG_REQUIRE(run_ptr[m] <= run_ptr[m + 1], "run_ptr non-decreasing");
    const size_t n_in = (size_t)C * N, n_out = (size_t)C * M;
    Staging st(device);
    return st.call(dig_map_windows, st.in(mu_cm, n_in), st.in(std_cm, n_in), st.in(y_cm, n_in), st.in(flag_cm, n_in), C, N,
                   st.in(run_ptr, M + 1), M, drop_flagged, tail, st.out(n_bins, n_out), st.out(y_true, n_out), st.out(y_pred, n_out),
                   st.out(std, n_out), st.out(pval, n_out), nullptr);
}

int dig_map_scores_host(const int32_t* n_bins, const int64_t* y_true, const double* y_pred, const double* pval, int64_t C, int64_t M,
                        int64_t* counts, double* sums, int device)
{
    int64_t chunks = 0;
    if (int rc = map_scores_sizes(__func__, C, M, &chunks)) return rc;
    if (C == 0) return DIG_OK;
    DIG_REQUIRE(counts && sums, "non-null counts, sums");
    const size_t n = (size_t)C * M;
    DIG_REQUIRE(n == 0 || (n_bins && y_true && y_pred && pval), "non-null n_bins, y_true, y_pred, pval");
    const int64_t wsb = dig_map_scores_workspace(C, M);
    Staging st(device);
    return st.call(dig_map_scores, st.in(n_bins, n), st.in(y_true, n), st.in(y_pred, n), st.in(pval, n), C, M, st.out(counts, (size_t)C * 7),
                   st.out(sums, (size_t)C * 4), st.scratch((size_t)wsb), wsb, nullptr);
}

// what the twins of dig_pair_fisher / dig_pair_counts require of the plan arrays, which the device forms cannot look at
static int check_pair_plan(const char* fn, int64_t H_total, const int64_t* row_ptr, const int32_t* n_samples, const int64_t* pair_ptr,
                           int64_t C, const int32_t* tiles, int64_t n_tiles, int64_t n_pairs, int32_t n_max, int32_t h_max)
{
    DIG_REQUIRE_IN(fn, C == 0 || (row_ptr && n_samples && pair_ptr), "non-null row_ptr, n_samples, pair_ptr");
    DIG_REQUIRE_IN(fn, n_tiles == 0 || (tiles && C > 0), "non-null tiles");
    if (C == 0) {
        DIG_REQUIRE_IN(fn, H_total == 0 && n_pairs == 0, "no row and no pair without a cohort");
        return DIG_OK;
    }
    DIG_REQUIRE_IN(fn, row_ptr[0] == 0 && row_ptr[C] == H_total, "row_ptr: 0 first, H_total last");
    DIG_REQUIRE_IN(fn, pair_ptr[0] == 0 && pair_ptr[C] == n_pairs, "pair_ptr: 0 first, n_pairs last");
    for (int64_t c = 0; c < C; ++c) {
        const int64_t H = row_ptr[c + 1] - row_ptr[c];
        DIG_REQUIRE_IN(fn, H >= 0 && H <= h_max, "0 <= rows of a cohort <= h_max");
        DIG_REQUIRE_IN(fn, n_samples[c] >= 0 && n_samples[c] <= n_max, "0 <= n_samples <= n_max");
        DIG_REQUIRE_IN(fn, pair_ptr[c + 1] - pair_ptr[c] == H * (H - 1) / 2, "pair_ptr: H (H - 1) / 2 pairs per cohort");
    }
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int32_t c = tiles[3 * t], bi = tiles[3 * t + 1], bj = tiles[3 * t + 2];
        DIG_REQUIRE_IN(fn, c >= 0 && c < C && bi >= 0 && bi <= bj && (int64_t)bj * DIG_PAIR_TILE < row_ptr[c + 1] - row_ptr[c],
                       "tiles: (cohort, block i <= block j) inside the cohort's rows");
    }
    return DIG_OK;
}

int dig_pair_bits_host(const int32_t* row, const int32_t* sample, int64_t n_keys, int64_t H_total, int64_t W, uint64_t* bits, int device)
{
    unsigned blocks = 0;
    if (int rc = pair_bits_sizes(__func__, n_keys, H_total, W, bits, &blocks)) return rc;
    if (H_total == 0) return DIG_OK;
    DIG_REQUIRE(n_keys == 0 || (row && sample), "non-null row, sample");
    Staging st(device);
    return st.call(dig_pair_bits, st.in(row, n_keys), st.in(sample, n_keys), n_keys, H_total, W, st.out(bits, (size_t)H_total * W), nullptr);
}

int dig_pair_fisher_host(const uint64_t* bits, int64_t H_total, int64_t W, const int64_t* row_ptr, const int32_t* n_samples,
                         const int64_t* pair_ptr, int64_t C, const int32_t* tiles, int64_t n_tiles, int64_t n_pairs, int32_t n_max,
                         int32_t h_max, double* lnfact, int32_t* n_row, int32_t* n_both, double* pval_cooccur, double* pval_exclusive,
                         int device)
{
    if (int rc = pair_fisher_sizes(__func__, bits, H_total, W, C, n_tiles, n_pairs, n_max, h_max)) return rc;
    DIG_REQUIRE(lnfact, "non-null lnfact");
    DIG_REQUIRE(H_total == 0 || n_row, "non-null n_row");
    DIG_REQUIRE(n_pairs == 0 || (n_both && pval_cooccur && pval_exclusive), "non-null n_both, pval_cooccur, pval_exclusive");
    if (int rc = check_pair_plan(__func__, H_total, row_ptr, n_samples, pair_ptr, C, tiles, n_tiles, n_pairs, n_max, h_max)) return rc;
    Staging st(device);
    return st.call(dig_pair_fisher, st.in(bits, (size_t)H_total * W), H_total, W, st.in(row_ptr, C + 1), st.in(n_samples, C),
                   st.in(pair_ptr, C + 1), C, st.in(tiles, 3 * n_tiles), n_tiles, n_pairs, n_max, h_max, st.out(lnfact, (size_t)n_max + 1),
                   st.out(n_row, H_total), st.out(n_both, n_pairs), st.out(pval_cooccur, n_pairs), st.out(pval_exclusive, n_pairs),
                   nullptr);
}

int dig_pair_counts_host(const uint64_t* bits, int64_t H_total, int64_t W, const int64_t* row_ptr, const int32_t* n_samples,
                         const int64_t* pair_ptr, int64_t C, const int32_t* tiles, int64_t n_tiles, int64_t n_pairs, int32_t n_max,
                         int32_t h_max, int32_t* n_row, int32_t* n_both, int device)
{
    if (int rc = pair_fisher_sizes(__func__, bits, H_total, W, C, n_tiles, n_pairs, n_max, h_max)) return rc;
    DIG_REQUIRE(H_total == 0 || n_row, "non-null n_row");
    DIG_REQUIRE(n_pairs == 0 || n_both, "non-null n_both");
    if (int rc = check_pair_plan(__func__, H_total, row_ptr, n_samples, pair_ptr, C, tiles, n_tiles, n_pairs, n_max, h_max)) return rc;
    Staging st(device);
    return st.call(dig_pair_counts, st.in(bits, (size_t)H_total * W), H_total, W, st.in(row_ptr, C + 1), st.in(n_samples, C),
                   st.in(pair_ptr, C + 1), C, st.in(tiles, 3 * n_tiles), n_tiles, n_pairs, n_max, h_max, st.out(n_row, H_total),
                   st.out(n_both, n_pairs), nullptr);
}

int dig_scale_suffstats_host(const double* bin_mu, const uint8_t* bin_flag, int64_t N, int64_t C, double* out_sum, int device)
{
    DIG_REQUIRE(N >= 0 && C >= 0, "N, C >= 0");
    if (C == 0) return DIG_OK;
    DIG_REQUIRE(out_sum, "non-null output");
    const size_t n = (size_t)N * C;
    DIG_REQUIRE(n == 0 || (bin_mu && bin_flag), "non-null inputs");
    const int64_t wsb = dig_scale_suffstats_workspace(N, C);
    Staging st(device);
    return st.call(dig_scale_suffstats, st.in(bin_mu, n), st.in(bin_flag, n), N, C, st.out(out_sum, C), st.scratch((size_t)wsb), wsb,
                   nullptr);
}

int dig_gather_bins_host(const void* x_data, int src_dtype, int64_t N, int64_t L, int64_t T, const int64_t* bin_rows, int64_t B,
                         const int32_t* tracks, int64_t T_sel, void* out, int out_dtype, int transpose_out, int device)
{
    DIG_REQUIRE(N >= 0 && L > 0 && T > 0 && B >= 0 && T_sel >= 0, "sizes");
    if (B == 0 || T_sel == 0) return DIG_OK;
    DIG_REQUIRE(x_data && bin_rows && out, "non-null pointers");
    DIG_REQUIRE(tracks || T_sel == T, "tracks == NULL selects all tracks: T_sel must equal T");
    const size_t ss = dtype_size(src_dtype), ds = dtype_size(out_dtype);
    DIG_REQUIRE(ss && ds, "known dtypes");
    for (int64_t b = 0; b < B; ++b) DIG_REQUIRE(bin_rows[b] >= 0 && bin_rows[b] < N, "bin_rows within [0, N)");
    for (int64_t t = 0; tracks && t < T_sel; ++t) DIG_REQUIRE(tracks[t] >= 0 && tracks[t] < T, "tracks within [0, T)");
    Staging st(device);
    return st.call(dig_gather_bins, st.in_bytes(x_data, (size_t)N * L * T * ss), src_dtype, N, L, T, st.in(bin_rows, B), B,
                   st.in(tracks, T_sel), T_sel, st.out_bytes(out, (size_t)B * L * T_sel * ds), out_dtype, transpose_out, nullptr);
}

int dig_count_contexts_host(const uint32_t* genome_words, int64_t n_words, const int64_t* chrom_off, const int64_t* chrom_len,
                            int n_chrom, const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end,
                            const uint8_t* reg_minus, int64_t R, int32_t* out, int device)
{
    DIG_REQUIRE(R >= 0 && n_words >= 2 && n_chrom >= 0, "R >= 0, n_words >= 2 (pad words), n_chrom >= 0");
    if (R == 0) return DIG_OK;
    DIG_REQUIRE(genome_words && chrom_off && chrom_len && reg_chrom && reg_start && reg_end && reg_minus && out,
                "non-null pointers");
    if (int rc = check_regions(__func__, reg_chrom, reg_start, reg_end, R, n_chrom)) return rc;
    for (int c = 0; c < n_chrom; ++c)
        DIG_REQUIRE((chrom_off[c] & 7) == 0 && chrom_off[c] + chrom_len[c] <= (n_words - 2) * 8,
                    "chromosomes word-aligned and inside the genome array");
    const size_t nc = std::max(n_chrom, 1);
    Staging st(device);
    return st.call(dig_count_contexts, st.in(genome_words, n_words), n_words, st.in(chrom_off, nc), st.in(chrom_len, nc), n_chrom,
                   st.in(reg_chrom, R), st.in(reg_start, R), st.in(reg_end, R), st.in(reg_minus, R), R, st.out(out, (size_t)R * 64),
                   nullptr);
}

int dig_count_contexts2_host(const uint32_t* words2, int64_t n_words2, const int64_t* nint_start, const int64_t* nint_end, int64_t n_int,
                             const int32_t* nint_bucket, int64_t n_buckets, const int64_t* chrom_off, const int64_t* chrom_len,
                             int n_chrom, const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end,
                             const uint8_t* reg_minus, int64_t R, int32_t* out, int device)
{
    const Genome2 H = {words2, n_words2, nint_start, nint_end, n_int, nint_bucket, n_buckets, chrom_off, chrom_len, n_chrom};
    if (int rc = genome2_check(__func__, H, R, true)) return rc;
    if (R == 0) return DIG_OK;
    DIG_REQUIRE(words2 && chrom_off && chrom_len && reg_chrom && reg_start && reg_end && reg_minus && out, "non-null pointers");
    if (int rc = check_regions(__func__, reg_chrom, reg_start, reg_end, R, n_chrom)) return rc;
    if (int rc = genome2_check_host(__func__, H)) return rc;
    Staging st(device);
    return call_genome2(st, dig_count_contexts2, H, st.in(reg_chrom, R), st.in(reg_start, R), st.in(reg_end, R), st.in(reg_minus, R), R,
                        st.out(out, (size_t)R * 64), nullptr);
}

int dig_count_contexts5_host(const uint32_t* words2, int64_t n_words2, const int64_t* nint_start, const int64_t* nint_end, int64_t n_int,
                             const int32_t* nint_bucket, int64_t n_buckets, const int64_t* chrom_off, const int64_t* chrom_len,
                             int n_chrom, const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end,
                             const uint8_t* reg_minus, int64_t R, int32_t* out, int device)
{
    const Genome2 H = {words2, n_words2, nint_start, nint_end, n_int, nint_bucket, n_buckets, chrom_off, chrom_len, n_chrom};
    if (int rc = genome2_check(__func__, H, R, true)) return rc;
    if (R == 0) return DIG_OK;
    DIG_REQUIRE(words2 && chrom_off && chrom_len && reg_chrom && reg_start && reg_end && reg_minus && out, "non-null pointers");
    if (int rc = check_regions(__func__, reg_chrom, reg_start, reg_end, R, n_chrom)) return rc;
    for (int64_t r = 0; r < R; ++r)
        DIG_REQUIRE(reg_start[r] == 0 || reg_start[r] >= 2, "START 0 or >= 2 (the fetch would start before the chromosome)");
    if (int rc = genome2_check_host(__func__, H)) return rc;
    Staging st(device);
    return call_genome2(st, dig_count_contexts5, H, st.in(reg_chrom, R), st.in(reg_start, R), st.in(reg_end, R), st.in(reg_minus, R), R,
                        st.out(out, (size_t)R * 1024), nullptr);
}

int dig_mutation_contexts_host(const uint32_t* words2, int64_t n_words2, const int64_t* nint_start, const int64_t* nint_end, int64_t n_int,
                               const int32_t* nint_bucket, int64_t n_buckets, const int64_t* chrom_off, const int64_t* chrom_len,
                               int n_chrom, const int32_t* row_chrom, const int64_t* row_start, const uint8_t* row_ref, int64_t n_rows,
                               int n_up, int n_down, int collapse, uint8_t* status, uint32_t* context, int device)
{
    DIG_REQUIRE(n_rows >= 0 && n_rows <= INT32_MAX, "0 <= n_rows < 2^31");
    DIG_REQUIRE(n_up >= 0 && n_down >= 0 && n_up + n_down + 1 <= 16, "n_up, n_down >= 0 and n_up + n_down + 1 <= 16");
    const Genome2 H = {words2, n_words2, nint_start, nint_end, n_int, nint_bucket, n_buckets, chrom_off, chrom_len, n_chrom};
    if (int rc = genome2_check(__func__, H, n_rows)) return rc;
    if (n_rows == 0) return DIG_OK;
    DIG_REQUIRE(words2 && chrom_off && chrom_len && row_chrom && row_start && row_ref && status && context, "non-null pointers");
    for (int64_t r = 0; r < n_rows; ++r) DIG_REQUIRE(row_chrom[r] >= 0 && row_chrom[r] < n_chrom, "row chromosome index within [0, n_chrom)");
    if (int rc = genome2_check_host(__func__, H)) return rc;
    const int64_t ws = dig_mutation_contexts_workspace(n_rows);
    Staging st(device);
    return call_genome2(st, dig_mutation_contexts, H, st.in(row_chrom, n_rows), st.in(row_start, n_rows), st.in(row_ref, n_rows), n_rows,
                        n_up, n_down, collapse, st.out(status, n_rows), st.out(context, n_rows), st.scratch(ws), ws, nullptr);
}

int dig_mutation_function_host(const uint32_t* words2, int64_t n_words2, const int64_t* nint_start, const int64_t* nint_end, int64_t n_int,
                               const int32_t* nint_bucket, int64_t n_buckets, const int64_t* chrom_off, const int64_t* chrom_len,
                               int n_chrom, const int32_t* gene_chrom, const uint8_t* gene_minus, const int64_t* blk_ptr,
                               const int64_t* blk_start, const int64_t* blk_end, const int64_t* cds_off, const int64_t* spl_ptr,
                               const int64_t* spl_pos, int64_t n_genes, const int32_t* pair_gene, const int64_t* pair_start,
                               const int64_t* pair_end, const uint8_t* pair_kind, const uint8_t* pair_ref, const uint8_t* pair_alt,
                               int64_t n_pairs, uint8_t* impact, uint8_t* status, int32_t* n_cds, int32_t* cds_min, int32_t* cds_max,
                               int device)
{
    DIG_REQUIRE(n_pairs >= 0 && n_genes >= 0, "n_pairs, n_genes >= 0");
    const Genome2 H = {words2, n_words2, nint_start, nint_end, n_int, nint_bucket, n_buckets, chrom_off, chrom_len, n_chrom};
    if (int rc = genome2_check(__func__, H, n_pairs)) return rc;
    if (n_pairs == 0) return DIG_OK;
    DIG_REQUIRE(words2 && chrom_off && chrom_len && blk_ptr && spl_ptr, "non-null genome arrays, blk_ptr, spl_ptr");
    DIG_REQUIRE(pair_gene && pair_start && pair_end && pair_kind && pair_ref && pair_alt, "non-null pair arrays");
    DIG_REQUIRE(impact && status && n_cds && cds_min && cds_max, "non-null outputs");
    const int64_t n_blk = blk_ptr[n_genes], n_spl = spl_ptr[n_genes];
    DIG_REQUIRE(blk_ptr[0] == 0 && spl_ptr[0] == 0 && n_blk >= 0 && n_spl >= 0, "blk_ptr, spl_ptr start at 0");
    DIG_REQUIRE(n_genes == 0 || (gene_chrom && gene_minus), "non-null gene_chrom, gene_minus");
    DIG_REQUIRE(n_blk == 0 || (blk_start && blk_end && cds_off), "non-null block arrays");
    DIG_REQUIRE(n_spl == 0 || spl_pos, "non-null spl_pos");
    if (int rc = genome2_check_host(__func__, H)) return rc;
    if (int rc = check_gene_table(__func__, gene_chrom, blk_ptr, blk_start, blk_end, cds_off, spl_ptr, spl_pos, n_genes, chrom_len, n_chrom))
        return rc;
    for (int64_t i = 0; i < n_pairs; ++i) DIG_REQUIRE(pair_gene[i] >= 0 && pair_gene[i] < n_genes, "pair gene index within [0, n_genes)");
    const size_t ng = (size_t)n_genes;
    Staging st(device);
    return call_genome2(st, dig_mutation_function, H, st.in(gene_chrom, ng), st.in(gene_minus, ng), st.in(blk_ptr, ng + 1),
                        st.in(blk_start, n_blk), st.in(blk_end, n_blk), st.in(cds_off, n_blk), st.in(spl_ptr, ng + 1),
                        st.in(spl_pos, n_spl), n_genes, st.in(pair_gene, n_pairs), st.in(pair_start, n_pairs), st.in(pair_end, n_pairs),
                        st.in(pair_kind, n_pairs), st.in(pair_ref, n_pairs), st.in(pair_alt, n_pairs), n_pairs, st.out(impact, n_pairs),
                        st.out(status, n_pairs), st.out(n_cds, n_pairs), st.out(cds_min, n_pairs), st.out(cds_max, n_pairs), nullptr);
}

int dig_gene_site_counts_host(const uint32_t* words2, int64_t n_words2, const int64_t* nint_start, const int64_t* nint_end, int64_t n_int,
                              const int32_t* nint_bucket, int64_t n_buckets, const int64_t* chrom_off, const int64_t* chrom_len,
                              int n_chrom, const int32_t* gene_chrom, const uint8_t* gene_minus, const int64_t* blk_ptr,
                              const int64_t* blk_start, const int64_t* blk_end, const int64_t* cds_off, const int64_t* spl_ptr,
                              const int64_t* spl_pos, int64_t n_genes, int32_t* L, int32_t* n_stop_loss, uint8_t* status, int device)
{
    DIG_REQUIRE(n_genes >= 0, "n_genes >= 0");
    const Genome2 H = {words2, n_words2, nint_start, nint_end, n_int, nint_bucket, n_buckets, chrom_off, chrom_len, n_chrom};
    if (int rc = genome2_check(__func__, H, n_genes)) return rc;
    if (n_genes == 0) return DIG_OK;
    DIG_REQUIRE(words2 && chrom_off && chrom_len && blk_ptr && spl_ptr, "non-null genome arrays, blk_ptr, spl_ptr");
    DIG_REQUIRE(gene_chrom && gene_minus, "non-null gene_chrom, gene_minus");
    DIG_REQUIRE(L && n_stop_loss && status, "non-null outputs");
    const int64_t n_blk = blk_ptr[n_genes], n_spl = spl_ptr[n_genes];
    DIG_REQUIRE(blk_ptr[0] == 0 && spl_ptr[0] == 0 && n_blk >= 0 && n_spl >= 0, "blk_ptr, spl_ptr start at 0");
    DIG_REQUIRE(n_blk == 0 || (blk_start && blk_end && cds_off), "non-null block arrays");
    DIG_REQUIRE(n_spl == 0 || spl_pos, "non-null spl_pos");
    if (int rc = genome2_check_host(__func__, H)) return rc;
    if (int rc = check_gene_table(__func__, gene_chrom, blk_ptr, blk_start, blk_end, cds_off, spl_ptr, spl_pos, n_genes, chrom_len, n_chrom))
        return rc;
    const size_t ng = (size_t)n_genes;
    Staging st(device);
    return call_genome2(st, dig_gene_site_counts, H, st.in(gene_chrom, ng), st.in(gene_minus, ng), st.in(blk_ptr, ng + 1),
                        st.in(blk_start, n_blk), st.in(blk_end, n_blk), st.in(cds_off, n_blk), st.in(spl_ptr, ng + 1),
                        st.in(spl_pos, n_spl), n_genes, st.out(L, ng * 4 * 192), st.out(n_stop_loss, ng), st.out(status, ng), nullptr);
}

int dig_element_context_counts_host(const uint32_t* words2, int64_t n_words2, const int64_t* nint_start, const int64_t* nint_end,
                                    int64_t n_int, const int32_t* nint_bucket, int64_t n_buckets, const int64_t* chrom_off,
                                    const int64_t* chrom_len, int n_chrom, const int32_t* elt_chrom, const uint8_t* elt_minus,
                                    const int64_t* blk_ptr, const int64_t* blk_start, const int64_t* blk_end, int64_t E, int64_t n_blocks,
                                    int32_t* out, int device)
{
    DIG_REQUIRE(E >= 0 && n_blocks >= 0, "E, n_blocks >= 0");
    DIG_REQUIRE(E < ((int64_t)1 << 31) && n_blocks < ((int64_t)1 << 31), "E, n_blocks < 2^31");
    const Genome2 H = {words2, n_words2, nint_start, nint_end, n_int, nint_bucket, n_buckets, chrom_off, chrom_len, n_chrom};
    if (int rc = genome2_check(__func__, H, E)) return rc;
    if (E == 0) return DIG_OK;
    DIG_REQUIRE(words2 && chrom_off && chrom_len, "non-null genome arrays");
    DIG_REQUIRE(elt_chrom && elt_minus && blk_ptr && out, "non-null elt_chrom, elt_minus, blk_ptr, out");
    DIG_REQUIRE(((uintptr_t)out & 3) == 0, "out 4-byte aligned");
    DIG_REQUIRE(n_blocks == 0 || (blk_start && blk_end), "non-null blk_start, blk_end");
    DIG_REQUIRE(blk_ptr[0] == 0 && blk_ptr[E] == n_blocks, "blk_ptr from 0 to n_blocks");
    for (int64_t e = 0; e < E; ++e) {
        DIG_REQUIRE(blk_ptr[e] <= blk_ptr[e + 1], "blk_ptr non-decreasing");
        DIG_REQUIRE(elt_chrom[e] >= 0 && elt_chrom[e] < n_chrom, "element chromosome index within [0, n_chrom)");
    }
    for (int64_t b = 0; b < n_blocks; ++b) DIG_REQUIRE(blk_start[b] >= 0 && blk_end[b] >= 0, "non-negative coordinates");
    if (int rc = genome2_check_host(__func__, H)) return rc;
    const int64_t ws = dig_element_context_counts_workspace(n_blocks);
    const size_t ne = (size_t)E;
    Staging st(device);
    return call_genome2(st, dig_element_context_counts, H, st.in(elt_chrom, ne), st.in(elt_minus, ne), st.in(blk_ptr, ne + 1),
                        st.in(blk_start, n_blocks), st.in(blk_end, n_blocks), E, n_blocks, st.out(out, ne * 64), st.scratch(ws), ws,
                        nullptr);
}

int dig_element_pipeline_host(const double* bin_mu, const double* bin_std, const int32_t* bin_y, const uint8_t* bin_flag,
                              const int32_t* bin_ctx, const int64_t* ov_ptr, const int32_t* ov_idx, const int32_t* L,
                              const uint8_t* strand_minus, const int32_t* gene_length, const double* d_pr,
                              const int32_t* obs_snv, const int32_t* obs_samples, const int32_t* obs_indel, const double* cj,
                              const double* cj_indel, double* MU, double* SIGMA, int32_t* R_OBS, int32_t* FLAG, double* P,
                              int32_t* R_SIZE, int32_t* ELT_SIZE, double* P_INDEL, double* out, int64_t N, int64_t E, int64_t C,
                              int device)
{
    DIG_REQUIRE(N >= 0 && E >= 0 && C >= 0, "N, E, C >= 0");
    if (E == 0 || C == 0) return DIG_OK;
    DIG_REQUIRE(bin_mu && bin_std && bin_y && bin_flag && bin_ctx && ov_ptr && ov_idx && L && strand_minus && d_pr,
                "non-null accumulation inputs");
    DIG_REQUIRE(obs_snv && obs_samples && obs_indel && cj && cj_indel, "non-null statistics inputs");
    DIG_REQUIRE(MU && SIGMA && R_OBS && FLAG && P && R_SIZE && ELT_SIZE && P_INDEL && out, "non-null outputs");
    const int64_t nnz = ov_ptr[E];
    DIG_REQUIRE(nnz >= 0, "ov_ptr[E] >= 0");
    for (int64_t q = 0; q < nnz; ++q) DIG_REQUIRE(ov_idx[q] >= 0 && ov_idx[q] < N, "ov_idx within [0, N)");
    const int64_t wsb = dig_element_pipeline_workspace(E, C);
    DIG_REQUIRE(wsb > 0, "E * C must stay below 2^32 - 1");
    const size_t nNC = (size_t)N * C, nEC = (size_t)E * C;
    Staging st(device);
    const int32_t* dL = st.in(L, (size_t)E * 192);
    void* ws = st.scratch((size_t)wsb);
    int compact = 0;
    if (N >= 1) {
        if (int rc = st.staged()) return rc;
        if (int rc = dig_element_pipeline_prepare(dL, E, C, ws, wsb, &compact, nullptr)) return rc;
    }
    return st.call(dig_element_pipeline, st.in(bin_mu, nNC), st.in(bin_std, nNC), st.in(bin_y, nNC), st.in(bin_flag, nNC),
                   st.in(bin_ctx, (size_t)N * 64), st.in(ov_ptr, (size_t)E + 1), st.in(ov_idx, (size_t)(nnz > 0 ? nnz : 1)), dL,
                   st.in(strand_minus, E), st.in(gene_length, E), st.in(d_pr, (size_t)C * 192), st.in(obs_snv, nEC),
                   st.in(obs_samples, nEC), st.in(obs_indel, nEC), st.in(cj, C), st.in(cj_indel, C), st.out(MU, nEC),
                   st.out(SIGMA, nEC), st.out(R_OBS, nEC), st.out(FLAG, nEC), st.out(P, nEC), st.out(R_SIZE, E), st.out(ELT_SIZE, E),
                   st.out(P_INDEL, E), st.out(out, nEC * 7), N, E, C, nullptr, DIG_PIPE_ALL | (compact ? DIG_PIPE_COMPACT_L : 0),
                   ws, wsb, nullptr);
}

int dig_gene_pipeline_host(const double* bin_mu, const double* bin_std, const int32_t* bin_y, const uint8_t* bin_flag,
                           const int32_t* bin_ctx, const int64_t* ov_ptr, const int32_t* ov_idx, const int32_t* L,
                           const uint8_t* strand_minus, const int32_t* gene_length, const double* d_pr, const int32_t* obs,
                           const int32_t* n_samp, const double* cj, const double* t_indel, int with_indel, double* MU, double* SIGMA,
                           int32_t* R_OBS, int32_t* FLAG, double* P, int32_t* R_SIZE, int32_t* ELT_SIZE, double* P_INDEL, double* out,
                           int64_t N, int64_t G, int64_t C, int device)
{
    DIG_REQUIRE(N >= 0 && G >= 0 && C >= 0, "N, G, C >= 0");
    if (G == 0 || C == 0) return DIG_OK;
    DIG_REQUIRE(bin_mu && bin_std && bin_y && bin_flag && bin_ctx && ov_ptr && ov_idx && L && strand_minus && d_pr, "non-null accumulation inputs");
    DIG_REQUIRE(obs && n_samp && cj && (!with_indel || t_indel), "non-null statistics inputs");
    DIG_REQUIRE(MU && SIGMA && R_OBS && FLAG && P && R_SIZE && ELT_SIZE && P_INDEL && out, "non-null outputs");
    const int64_t nnz = ov_ptr[G];
    DIG_REQUIRE(nnz >= 0, "ov_ptr[G] >= 0");
    for (int64_t q = 0; q < nnz; ++q) DIG_REQUIRE(ov_idx[q] >= 0 && ov_idx[q] < N, "ov_idx within [0, N)");
    const size_t nNC = (size_t)N * C, nGC = (size_t)G * C;
    const int64_t wsb = dig_accumulate_workspace(G, C);
    Staging st(device);
    return st.call(dig_gene_pipeline, st.in(bin_mu, nNC), st.in(bin_std, nNC), st.in(bin_y, nNC), st.in(bin_flag, nNC),
                   st.in(bin_ctx, (size_t)N * 64), st.in(ov_ptr, (size_t)G + 1), st.in(ov_idx, (size_t)(nnz > 0 ? nnz : 1)),
                   st.in(L, (size_t)G * 4 * 192), st.in(strand_minus, G), st.in(gene_length, G), st.in(d_pr, (size_t)C * 192),
                   st.in(obs, nGC * 5), st.in(n_samp, nGC * 6), st.in(cj, C), st.in(t_indel, C), with_indel, st.out(MU, nGC),
                   st.out(SIGMA, nGC), st.out(R_OBS, nGC), st.out(FLAG, nGC), st.out(P, nGC * 4), st.out(R_SIZE, G),
                   st.out(ELT_SIZE, G), st.out(P_INDEL, G), st.out(out, nGC * 22), N, G, C, st.scratch((size_t)wsb), wsb, nullptr);
}

int dig_base_tile_probs_host(const uint32_t* genome_words, int64_t n_words, const int64_t* chrom_off, const int64_t* chrom_len,
                             int n_chrom, const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end, int64_t R,
                             const double* s_prob, int64_t C, int binsize, int64_t n_tiles, double* pt, int64_t* first_pos,
                             int32_t* n_valid, int device)
{
    const TileArgs a{{genome_words, n_words, chrom_off, chrom_len, n_chrom, reg_chrom, reg_start, reg_end, R}, s_prob, C, 1, binsize,
                     n_tiles, pt, first_pos, n_valid, nullptr};
    if (int rc = check_tile_tables_host(__func__, a, true)) return rc;
    if (R == 0) return DIG_OK;
    Staging st(device);
    return call_tile_genome(st, dig_base_tile_probs, a, binsize, n_tiles, st.out(pt, (size_t)C * R * n_tiles), st.out(first_pos, R),
                            st.out(n_valid, R), nullptr);
}

int dig_base_tile_probs_ctx_host(const uint32_t* genome_words, int64_t n_words, const int64_t* chrom_off, const int64_t* chrom_len,
                                 int n_chrom, const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end, int64_t R,
                                 const double* s_prob, int64_t C, int n_up, int binsize, int64_t n_tiles, double* pt,
                                 int64_t* first_pos, int32_t* n_valid, int device)
{
    const TileArgs a{{genome_words, n_words, chrom_off, chrom_len, n_chrom, reg_chrom, reg_start, reg_end, R}, s_prob, C, n_up, binsize,
                     n_tiles, pt, first_pos, n_valid, nullptr};
    if (int rc = check_tile_tables_host(__func__, a, true)) return rc;
    if (R == 0) return DIG_OK;
    Staging st(device);
    return call_tile_genome(st, dig_base_tile_probs_ctx, a, n_up, binsize, n_tiles, st.out(pt, (size_t)C * R * n_tiles), st.out(first_pos, R),
                            st.out(n_valid, R), nullptr);
}

int dig_tile_mut_counts_host(const int32_t* pair_mut, const int32_t* pair_reg, int64_t n_pairs, const int64_t* mut_start,
                             int64_t n_mut, const int32_t* mut_cohort, const int64_t* first_pos, const int32_t* n_valid,
                             int binsize, int64_t n_tiles, int64_t R, int64_t C, int32_t* k, int device)
{
    DIG_REQUIRE(n_pairs >= 0 && n_mut >= 0 && binsize >= 1 && n_tiles >= 0 && R >= 0 && C >= 0, "non-negative sizes, binsize >= 1");
    const size_t n = (size_t)C * R * n_tiles;
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(k && first_pos && n_valid, "non-null outputs / region tables");
    DIG_REQUIRE(n_pairs == 0 || (pair_mut && pair_reg && mut_start && mut_cohort), "non-null pair / mutation arrays");
    if (int rc = check_pairs_host(__func__, pair_mut, pair_reg, n_pairs, n_mut, R)) return rc;
    Staging st(device);
    return st.call(dig_tile_mut_counts, st.in(pair_mut, n_pairs), st.in(pair_reg, n_pairs), n_pairs, st.in(mut_start, n_mut),
                   st.in(mut_cohort, n_mut), st.in(first_pos, R), st.in(n_valid, R), binsize, n_tiles, R, C, st.out(k, n), nullptr);
}

int dig_tile_sample_keys_host(const int32_t* pair_mut, const int32_t* pair_reg, int64_t n_pairs, const int64_t* mut_start, int64_t n_mut,
                              const int32_t* mut_cohort, const int32_t* mut_sample, const uint8_t* keep, const int64_t* first_pos,
                              const int32_t* n_valid, int binsize, int64_t n_tiles, int64_t R, int64_t C, int64_t n_samples,
                              int64_t* keys, int device)
{
    DIG_REQUIRE(n_pairs >= 0 && n_mut >= 0 && binsize >= 1, "n_pairs, n_mut >= 0, binsize >= 1");
    int sb = 0;
    if (int rc = tile_sample_key_layout(__func__, C, R, n_tiles, n_samples, &sb)) return rc;
    if (n_pairs == 0) return DIG_OK;
    DIG_REQUIRE(pair_mut && pair_reg && keys, "non-null pair arrays, keys");
    DIG_REQUIRE(n_mut == 0 || (mut_start && mut_cohort && mut_sample), "non-null mutation arrays");
    DIG_REQUIRE(R == 0 || (first_pos && n_valid), "non-null region tables");
    if (int rc = check_pairs_host(__func__, pair_mut, pair_reg, n_pairs, n_mut, R)) return rc;
    for (int64_t m = 0; m < n_mut; ++m)
        DIG_REQUIRE(mut_cohort[m] < 0 || mut_cohort[m] >= C || (mut_sample[m] >= 0 && mut_sample[m] < n_samples),
                    "global sample within [0, n_samples) for every row of a cohort within [0, C)");
    Staging st(device);
    return st.call(dig_tile_sample_keys, st.in(pair_mut, n_pairs), st.in(pair_reg, n_pairs), n_pairs, st.in(mut_start, n_mut), n_mut,
                   st.in(mut_cohort, n_mut), st.in(mut_sample, n_mut), st.in(keep, n_samples), st.in(first_pos, R), st.in(n_valid, R),
                   binsize, n_tiles, R, C, n_samples, st.out(keys, n_pairs), nullptr);
}

int dig_tile_sample_counts_host(const int64_t* keys_sorted, int64_t n, int64_t C, int64_t R, int64_t n_tiles, int64_t n_samples,
                                int64_t cap, int32_t* k_cap, int32_t* k_samples, int device)
{
    DIG_REQUIRE(n >= 0 && n <= INT32_MAX, "0 <= n < 2^31 (the counts are 32-bit)");
    int sb = 0;
    if (int rc = tile_sample_key_layout(__func__, C, R, n_tiles, n_samples, &sb)) return rc;
    const size_t slots = (size_t)C * R * n_tiles;
    if (slots == 0 || (!k_cap && !k_samples)) return DIG_OK;
    DIG_REQUIRE(n == 0 || keys_sorted, "non-null keys");
    if (int rc = check_ascending(__func__, keys_sorted, n)) return rc;
    Staging st(device);
    // (a plane that is NULL is not staged: the call skips it)
    return st.call(dig_tile_sample_counts, st.in(keys_sorted, n), n, C, R, n_tiles, n_samples, cap, k_cap ? st.out(k_cap, slots) : nullptr,
                   k_samples ? st.out(k_samples, slots) : nullptr, nullptr);
}

int dig_tile_window_test_host(const double* pt, const int32_t* k, const double* mu, const double* sigma, const int32_t* n_valid,
                              int64_t C, int64_t R, int64_t T, int32_t width, double* pt_w, int32_t* k_w, double* exp_w,
                              double* pval_w, int32_t* n_windows, int device)
{
    if (int rc = tile_window_sizes(__func__, C, R, T, width)) return rc;
    const size_t rows = (size_t)C * R, n = rows * T;
    if (n == 0 || (!pt_w && !k_w && !exp_w && !pval_w && !n_windows)) return DIG_OK;
    DIG_REQUIRE(pt && k && mu && sigma && n_valid, "non-null pt, k, mu, sigma, n_valid");
    Staging st(device);
    // (an output that is NULL is not staged: the call skips it)
    return st.call(dig_tile_window_test, st.in(pt, n), st.in(k, n), st.in(mu, rows), st.in(sigma, rows), st.in(n_valid, R), C, R, T, width,
                   pt_w ? st.out(pt_w, n) : nullptr, k_w ? st.out(k_w, n) : nullptr, exp_w ? st.out(exp_w, n) : nullptr,
                   pval_w ? st.out(pval_w, n) : nullptr, n_windows ? st.out(n_windows, R) : nullptr, nullptr);
}

int dig_tile_window_sample_keys_host(const int64_t* keys, int64_t n, int64_t C, int64_t R, int64_t T, int64_t n_samples,
                                     int64_t* keys_out, int device)
{
    DIG_REQUIRE(n >= 0, "n >= 0");
    int sb = 0;
    if (int rc = tile_sample_key_layout(__func__, C, R, T, n_samples, &sb)) return rc;
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(keys && keys_out, "non-null keys, keys_out");
    Staging st(device);
    return st.call(dig_tile_window_sample_keys, st.in(keys, n), n, C, R, T, n_samples, st.out(keys_out, n), nullptr);
}

int dig_tile_window_samples_host(const int64_t* keys_sorted, int64_t n, const int32_t* n_valid, int64_t C, int64_t R, int64_t T,
                                 int64_t n_samples, int32_t width, int32_t* s_w, int device)
{
    if (int rc = tile_window_sizes(__func__, C, R, T, width)) return rc;
    DIG_REQUIRE(n >= 0 && n <= INT32_MAX, "0 <= n < 2^31 (the counts are 32-bit)");
    int sb = 0;
    if (int rc = tile_sample_key_layout(__func__, C, R, T, n_samples, &sb)) return rc;
    const size_t slots = (size_t)C * R * T;
    if (slots == 0) return DIG_OK;
    DIG_REQUIRE(s_w && n_valid && (n == 0 || keys_sorted), "non-null s_w, n_valid, keys");
    if (int rc = check_ascending(__func__, keys_sorted, n)) return rc;
    Staging st(device);
    return st.call(dig_tile_window_samples, st.in(keys_sorted, n), n, st.in(n_valid, R), C, R, T, n_samples, width, st.out(s_w, slots),
                   nullptr);
}

int dig_tile_census_host(const uint32_t* genome_words, int64_t n_words, const int64_t* chrom_off, const int64_t* chrom_len, int n_chrom,
                         const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end, int64_t R, const double* s_prob,
                         int64_t C, int n_up, int binsize, int64_t n_tiles, int64_t* first_pos, int32_t* n_valid, double* denom,
                         int32_t* n_positive, int device)
{
    const TileArgs a{{genome_words, n_words, chrom_off, chrom_len, n_chrom, reg_chrom, reg_start, reg_end, R}, s_prob, C, n_up, binsize,
                     n_tiles, nullptr, first_pos, n_valid, nullptr};
    if (int rc = check_tile_tables_host(__func__, a, false)) return rc;
    int64_t slots = 0;
    if (int rc = sparse_tile_slots(__func__, C, R, n_tiles, &slots)) return rc;
    if (R == 0) return DIG_OK;
    DIG_REQUIRE(first_pos && n_valid, "non-null first_pos, n_valid");
    DIG_REQUIRE(C == 0 || (s_prob && denom && n_positive), "non-null s_prob, denom, n_positive");
    const size_t rows = (size_t)C * R;
    const int64_t wsb = tile_census_workspace_bytes(C, n_up);
    Staging st(device);
    return call_tile_genome(st, dig_tile_census, a, n_up, binsize, n_tiles, st.out(first_pos, R), st.out(n_valid, R),
                            C ? st.out(denom, rows) : nullptr, C ? st.out(n_positive, rows) : nullptr, st.scratch(wsb), wsb, nullptr);
}

int dig_sparse_tile_keys_host(const int32_t* pair_mut, const int32_t* pair_reg, int64_t n_pairs, const int64_t* mut_start, int64_t n_mut,
                              const int32_t* mut_cohort, const int64_t* first_pos, const int32_t* n_valid, int binsize, int64_t n_tiles,
                              int64_t R, int64_t C, int64_t* keys, int device)
{
    DIG_REQUIRE(n_pairs >= 0 && n_mut >= 0 && binsize >= 1, "n_pairs, n_mut >= 0, binsize >= 1");
    int64_t slots = 0;
    if (int rc = sparse_tile_slots(__func__, C, R, n_tiles, &slots)) return rc;
    if (n_pairs == 0) return DIG_OK;
    DIG_REQUIRE(pair_mut && pair_reg && keys, "non-null pair arrays, keys");
    DIG_REQUIRE(n_mut == 0 || (mut_start && mut_cohort), "non-null mutation arrays");
    DIG_REQUIRE(R == 0 || (first_pos && n_valid), "non-null region tables");
    if (int rc = check_pairs_host(__func__, pair_mut, pair_reg, n_pairs, n_mut, R)) return rc;
    Staging st(device);
    return st.call(dig_sparse_tile_keys, st.in(pair_mut, n_pairs), st.in(pair_reg, n_pairs), n_pairs, st.in(mut_start, n_mut), n_mut,
                   st.in(mut_cohort, n_mut), st.in(first_pos, R), st.in(n_valid, R), binsize, n_tiles, R, C, st.out(keys, n_pairs), nullptr);
}

int dig_sparse_tile_test_host(const uint32_t* genome_words, int64_t n_words, const int64_t* chrom_off, const int64_t* chrom_len,
                              int n_chrom, const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end, int64_t R,
                              const double* s_prob, int64_t C, int n_up, int binsize, int64_t n_tiles, const double* denom,
                              const double* mu, const double* sigma, const int64_t* keys_sorted, int64_t n, int32_t* out_cohort,
                              int32_t* out_region, int32_t* out_tile, int32_t* out_k, double* out_pt, double* out_exp, double* out_pval,
                              int device)
{
    const TileArgs a{{genome_words, n_words, chrom_off, chrom_len, n_chrom, reg_chrom, reg_start, reg_end, R}, s_prob, C, n_up, binsize,
                     n_tiles, nullptr, nullptr, nullptr, nullptr};
    if (int rc = check_tile_tables_host(__func__, a, false)) return rc;
    DIG_REQUIRE(n >= 0 && n <= INT32_MAX, "0 <= n < 2^31 (the counts are 32-bit)");
    int64_t slots = 0;
    if (int rc = sparse_tile_slots(__func__, C, R, n_tiles, &slots)) return rc;
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(keys_sorted && out_cohort && out_region && out_tile && out_k && out_pt && out_exp && out_pval, "non-null keys and outputs");
    DIG_REQUIRE(slots == 0 || (s_prob && denom && mu && sigma), "non-null s_prob, denom, mu, sigma");
    if (int rc = check_ascending(__func__, keys_sorted, n)) return rc;
    const size_t rows = (size_t)C * R;
    Staging st(device);
    return call_tile_genome(st, dig_sparse_tile_test, a, n_up, binsize, n_tiles, st.in(denom, rows), st.in(mu, rows), st.in(sigma, rows),
                            st.in(keys_sorted, n), n, st.out(out_cohort, n), st.out(out_region, n), st.out(out_tile, n), st.out(out_k, n),
                            st.out(out_pt, n), st.out(out_exp, n), st.out(out_pval, n), nullptr);
}

int dig_tile_window_census_host(const uint32_t* genome_words, int64_t n_words, const int64_t* chrom_off, const int64_t* chrom_len,
                                int n_chrom, const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end, int64_t R,
                                const double* s_prob, int64_t C, int n_up, int binsize, int64_t n_tiles, int32_t width,
                                const int32_t* n_positive, int32_t* n_windows, int32_t* n_positive_w, int device)
{
    const TileArgs a{{genome_words, n_words, chrom_off, chrom_len, n_chrom, reg_chrom, reg_start, reg_end, R}, s_prob, C, n_up, binsize,
                     n_tiles, nullptr, nullptr, nullptr, nullptr};
    if (int rc = check_tile_tables_host(__func__, a, false)) return rc;
    int64_t slots = 0;
    if (int rc = sparse_window_sizes(__func__, C, R, n_tiles, width, &slots)) return rc;
    if (R == 0) return DIG_OK;
    DIG_REQUIRE(n_windows, "non-null n_windows");
    DIG_REQUIRE(C == 0 || (s_prob && n_positive_w), "non-null s_prob, n_positive_w");
    const size_t rows = (size_t)C * R;
    const int64_t wsb = tile_census_workspace_bytes(C, n_up);
    Staging st(device);
    return call_tile_genome(st, dig_tile_window_census, a, n_up, binsize, n_tiles, width, st.in(n_positive, rows), st.out(n_windows, R),
                            C ? st.out(n_positive_w, rows) : nullptr, st.scratch(wsb), wsb, nullptr);
}

int dig_sparse_window_count_host(const int64_t* keys_sorted, int64_t n, const int32_t* n_valid, int64_t C, int64_t R, int64_t T,
                                 int32_t width, int64_t* counts, int device)
{
    DIG_REQUIRE(n >= 0, "n >= 0");
    int64_t slots = 0;
    if (int rc = sparse_window_sizes(__func__, C, R, T, width, &slots)) return rc;
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(keys_sorted && counts, "non-null keys, counts");
    DIG_REQUIRE(slots == 0 || n_valid, "non-null n_valid");
    if (int rc = check_ascending(__func__, keys_sorted, n)) return rc;
    Staging st(device);
    return st.call(dig_sparse_window_count, st.in(keys_sorted, n), n, st.in(n_valid, R), C, R, T, width, st.out(counts, n), nullptr);
}

int dig_sparse_window_test_host(const uint32_t* genome_words, int64_t n_words, const int64_t* chrom_off, const int64_t* chrom_len,
                                int n_chrom, const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end, int64_t R,
                                const double* s_prob, int64_t C, int n_up, int binsize, int64_t n_tiles, const double* denom,
                                const double* mu, const double* sigma, const int64_t* keys_sorted, int64_t n, const int64_t* offsets,
                                int32_t width, int64_t w_begin, int64_t w_count, int32_t* out_cohort, int32_t* out_region,
                                int32_t* out_window, int32_t* out_k, double* out_pt, double* out_exp, double* out_pval, int device)
{
    const TileArgs a{{genome_words, n_words, chrom_off, chrom_len, n_chrom, reg_chrom, reg_start, reg_end, R}, s_prob, C, n_up, binsize,
                     n_tiles, nullptr, nullptr, nullptr, nullptr};
    if (int rc = check_tile_tables_host(__func__, a, false)) return rc;
    int64_t slots = 0;
    if (int rc = sparse_window_sizes(__func__, C, R, n_tiles, width, &slots)) return rc;
    DIG_REQUIRE(n >= 0 && w_begin >= 0 && w_count >= 0 && w_count <= INT32_MAX, "n, w_begin >= 0, 0 <= w_count < 2^31");
    if (w_count == 0) return DIG_OK;
    DIG_REQUIRE(offsets && out_cohort && out_region && out_window && out_k && out_pt && out_exp && out_pval, "non-null offsets and outputs");
    DIG_REQUIRE(n == 0 || keys_sorted, "non-null keys");
    DIG_REQUIRE(slots == 0 || n == 0 || (s_prob && denom && mu && sigma), "non-null s_prob, denom, mu, sigma");
    if (int rc = check_ascending(__func__, keys_sorted, n)) return rc;
    DIG_REQUIRE(offsets[0] == 0, "offsets: the exclusive prefix sum of the counts (0 first)");
    for (int64_t i = 0; i < n; ++i) DIG_REQUIRE(offsets[i] <= offsets[i + 1], "offsets: the exclusive prefix sum of the counts (non-decreasing)");
    const size_t rows = (size_t)C * R;
    Staging st(device);
    return call_tile_genome(st, dig_sparse_window_test, a, n_up, binsize, n_tiles, st.in(denom, rows), st.in(mu, rows), st.in(sigma, rows),
                            st.in(keys_sorted, n), n, st.in(offsets, n + 1), width, w_begin, w_count, st.out(out_cohort, w_count),
                            st.out(out_region, w_count), st.out(out_window, w_count), st.out(out_k, w_count), st.out(out_pt, w_count),
                            st.out(out_exp, w_count), st.out(out_pval, w_count), nullptr);
}

int dig_overlap_join_count_host(const int64_t* blk_start_key, const int64_t* blk_runmax_key, const int64_t* blk_end, int64_t n_blk,
                                const int64_t* mut_chrom, const int64_t* mut_start, const int64_t* mut_end, int64_t n_mut,
                                int32_t* counts, int device)
{
    DIG_REQUIRE(n_blk >= 0 && n_mut >= 0, "sizes >= 0");
    if (n_mut == 0) return DIG_OK;
    DIG_REQUIRE(mut_chrom && mut_start && mut_end && counts, "non-null mutation arrays");
    DIG_REQUIRE(n_blk == 0 || (blk_start_key && blk_runmax_key && blk_end), "non-null block arrays");
    Staging st(device);
    return st.call(dig_overlap_join_count, st.in(blk_start_key, n_blk), st.in(blk_runmax_key, n_blk), st.in(blk_end, n_blk), n_blk,
                   st.in(mut_chrom, n_mut), st.in(mut_start, n_mut), st.in(mut_end, n_mut), n_mut, st.out(counts, n_mut), nullptr);
}

int dig_overlap_join_fill_host(const int64_t* blk_start_key, const int64_t* blk_runmax_key, const int64_t* blk_end, int64_t n_blk,
                               const int64_t* mut_chrom, const int64_t* mut_start, const int64_t* mut_end, int64_t n_mut,
                               const int64_t* offsets, int64_t n_pairs, int32_t* pair_mut, int32_t* pair_blk, int device)
{
    DIG_REQUIRE(n_blk >= 0 && n_mut >= 0 && n_pairs >= 0, "sizes >= 0");
    if (n_mut == 0 || n_blk == 0 || n_pairs == 0) return DIG_OK;
    DIG_REQUIRE(mut_chrom && mut_start && mut_end && offsets && pair_mut && pair_blk, "non-null arrays");
    DIG_REQUIRE(blk_start_key && blk_runmax_key && blk_end, "non-null block arrays");
    Staging st(device);
    return st.call(dig_overlap_join_fill, st.in(blk_start_key, n_blk), st.in(blk_runmax_key, n_blk), st.in(blk_end, n_blk), n_blk,
                   st.in(mut_chrom, n_mut), st.in(mut_start, n_mut), st.in(mut_end, n_mut), n_mut, st.in(offsets, n_mut),
                   st.out(pair_mut, n_pairs), st.out(pair_blk, n_pairs), nullptr);
}

}  // extern "C"
