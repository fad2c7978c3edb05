// Shared declarations for the gfx950 kernels and the C-ABI host layer (internal; not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include <atomic>
#include <initializer_list>
#include <mutex>
#include "sf_base.h"

#define SF_LEAF 64        // Cholesky leaf block (potrf / trsm granularity); matrices padded to it
#define SF_NB 256         // outer left-looking panel width
#define SF_LS_MAXP SF_LOCAL_SCAN_MAX_PATCH  // widest patch of a local-scan candidate in pixels (sf_local_scan.h)
#define SF_MAX_LOCAL 32   // local kernels per model (sf_fill_elem.h: 32-bit masks of the fill tiles, per-block tables)
#define SF_NF_MIN_VSINI 16     // FFT lengths of a model with vsini: k_spline_apply takes whole 16-point blocks,
#define SF_NF_MAX_VSINI 65536  // sf_launch_broaden transforms at most 65536 points

typedef double sf_d4 __attribute__((ext_vector_type(4)));

#define SF_HIP(call)                                                                     \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            sf_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return SF_EHIP;                                                              \
        }                                                                                \
    } while (0)

#define SF_LAUNCH_CHECK()                                                                \
    do {                                                                                 \
        hipError_t e_ = hipGetLastError();                                               \
        if (e_ != hipSuccess) {                                                          \
            sf_set_error("%s:%d launch -> %s", __FILE__, __LINE__, hipGetErrorString(e_)); \
            return SF_EHIP;                                                              \
        }                                                                                \
    } while (0)

static inline size_t sf_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Function attributes (dynamic LDS limit) are per device, and contexts may be driven from different host threads:
// a call site owns one sf_dev_once; the set-up of a device runs once, under the site's mutex, and the device is
// marked only AFTER it succeeded (a second thread never launches before the attribute is in place).
struct sf_dev_once {
    std::atomic<unsigned long long> done{0};  // bitmask of the devices that are set up
    std::mutex mu;
};
template <class F>
static inline int sf_once_per_device(sf_dev_once* once, F&& setup) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return setup();
    const unsigned long long bit = 1ull << dev;
    if (once->done.load(std::memory_order_acquire) & bit) return SF_OK;
    std::lock_guard<std::mutex> lk(once->mu);
    if (once->done.load(std::memory_order_relaxed) & bit) return SF_OK;
    const int rc = setup();
    if (rc == SF_OK) once->done.fetch_or(bit, std::memory_order_release);
    return rc;
}
// the usual set-up: raise the dynamic LDS limit of `kernels` (in order) to `bytes`
static inline int sf_lds_limit_once(sf_dev_once* once, int bytes, std::initializer_list<const void*> kernels) {
    return sf_once_per_device(once, [&]() -> int {
        for (const void* k : kernels) SF_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        return SF_OK;
    });
}
#define SF_CHECK(expr)              \
    do {                            \
        const int rc_ = (expr);     \
        if (rc_ != SF_OK) return rc_; \
    } while (0)

// Tuning / test switches read from the environment exist ONLY in -DSF_TUNING builds (`make TUNING=1` ->
// libstarfish_amd_tuning.so, loaded by tools/ through SF_LIB_PATH).  The release library has no environment-dependent
// behaviour: the macros collapse to their defaults and the switch names do not appear in the binary.
#ifdef SF_TUNING
#define SF_TUNE_FLAG(name) (getenv(name) != nullptr)
#define SF_TUNE_INT(name, dflt) (getenv(name) ? atoi(getenv(name)) : (dflt))
#define SF_TUNE_STR(name) (static_cast<const char*>(getenv(name)))
#else
#define SF_TUNE_FLAG(name) (false)
#define SF_TUNE_INT(name, dflt) (dflt)
#define SF_TUNE_STR(name) (static_cast<const char*>(nullptr))
#endif

// Streams and events a launch sequence needs besides the caller's stream.  Owned by a context (sf_ctx) or,
// for the context-free entry points, by the calling thread -- the library keeps no process-global stream state,
// so contexts can be driven from different host threads (and devices) concurrently.
#ifndef SF_EXEC_GROUPS
#define SF_EXEC_GROUPS 2
#endif
static_assert(SF_EXEC_GROUPS >= 2, "the wide sequence and the multi-order lanes use grp[0]: at least two slab groups");
// streams the slab groups of the fused Cholesky are spread over (the caller's + 1; measured: 1 -> 54.8, 2 -> 52.9, 3 -> 53.8 ms at cfg 2)
struct sf_exec {
    int device = -1;
    hipStream_t side = nullptr;  // highest priority: the diagonal-block chain of the Cholesky
    hipStream_t grp[SF_EXEC_GROUPS - 1] = {};  // slab groups 1.. of the fused Cholesky (group 0 = caller's stream)
    hipStream_t aux = nullptr;   // banded path: band fill beside the transforms; multi-order calls: the fills
    hipEvent_t fork = nullptr, join = nullptr;
    hipEvent_t* pool = nullptr;
    size_t pool_size = 0, pool_cap = 0, used = 0;
};
int sf_exec_prepare(sf_exec* ex);               // streams of the CURRENT device (created on first use), pool rewound
int sf_exec_event(sf_exec* ex, hipEvent_t* e);  // next pooled event (timing disabled)
void sf_exec_release(sf_exec* ex);
sf_exec* sf_exec_thread_local(void);

// profiling hooks (sf_prof.cpp)
void sf_prof_gemm_begin(hipStream_t s, double flops, void** tok);
void sf_prof_gemm_end(void* tok);

// ---- launchers implemented in the .hip files (all enqueue on `s`, never synchronise) ----------
// sf_chol.hip
#define SF_LTB_DOUBLES (SF_LEAF * SF_LEAF + SF_LEAF)  // reserved per matrix at the start of the workspace (unused)
#define SF_LDT (SF_NB + 16)                            // row stride of the panel scratch
size_t sf_potrf_work_doubles(int n, int batch);        // doubles of scratch sf_launch_potrf needs
// Optional "matrix-free" start of the factorisation: 128x128 tiles whose tilemap byte is 0 were never
// written to A; their initial value is the rank-m product Y^T Y and is generated in the MFMA kernel.
struct sf_gen_args {
    const double* Y;  // [batch][mpad][ldy]
    int mpad, ldy;
    const unsigned char* tilemap;  // [batch][nt128 * nt128]
    int nt128;
    int fp;  // front pad the tile map was built for (sf_potrf_front_pad): tiles are those of the SHIFTED frame
};
// Orders whose padded size is an odd multiple of 64 (3008 = 23.5 slabs of 128 rows) are factorised in a frame shifted by
// `fp` = 64 virtual identity rows / columns IN FRONT: the half-empty slab becomes the first one, whose workgroups have
// the shortest K loops, instead of the last one with the longest (cfg 3: 6 % of the chip's time).  Nothing moves in
// memory: the kernels address the matrix from a base pointer fp (lda + 1) elements earlier, skip the fp leading columns
// of every K loop (they hold zeros below the diagonal block) and predicate the few accesses of the first tile row /
// column that would touch the virtual part.  0 = frame not shifted (n a multiple of 128, or the unfused sequence).
int sf_potrf_front_pad(int n, int batch);
int sf_launch_potrf(double* A, int n, int lda, int64_t stride, int batch, int* info, double* work,
                    double* rhs, int ldr, hipStream_t s, const sf_gen_args* gen = nullptr, sf_exec* ex = nullptr);
int sf_band_tiles_lda(int nband);
size_t sf_band_tiles_doubles(int nband, int batch);
int sf_band_tiles_wt(int halfwidth);  // tile (i, j) of a bordered band matrix meets the band iff i - j <= wt
int sf_set_persistent_potrf(int enable);  // 0 / 1: the dataflow sequence may be chosen; < 0: query.  Returns the previous value
int sf_persistent_potrf_read_status(long long* out8);  // sf_persistent_potrf_status (include/starfish_amd.h)
int sf_set_cholesky_sequence(int mode);  // -1 automatic (by batch size), 0 fused panel kernel, 1 unfused
int sf_launch_logdet_z(const double* L, int n, int lda, int64_t stride, int batch, const double* z, int ldr,
                       double* logdet, double* sqmah, hipStream_t s);
int sf_launch_logdet_sqmah(const double* L, int n, int lda, int64_t stride, int batch,
                           const double* R, int ldr, double* zscratch, double* logdet, double* sqmah, hipStream_t s);
// the factor applied to nrhs right-hand sides per matrix (op: SF_APPLY_*; layouts: sf_potrs_batch); arguments checked by the caller
int sf_launch_chol_apply(const double* L, int n, int lda, int64_t stride, int batch, int op, const double* rhs, int nrhs,
                         int ldr, int64_t rhs_stride, double* out, int ldo, int64_t out_stride, hipStream_t s);
// sf_apply_batch: right-hand sides (or, rhs NULL, the residuals [batch][npad]) into the staging area [batch][nrhs][npad],
// zero on the padding; its n data rows out again, NaN where info[b] != 0
int sf_launch_apply_stage(const double* rhs, int ldr, int64_t rhs_stride, const double* resid, int n, int npad, int nrhs,
                          int batch, double* stage, hipStream_t s);
int sf_launch_apply_export(const double* stage, const int* info, int n, int npad, int nrhs, int batch, double* out,
                           hipStream_t s);
// diag(C^-1) of the factored matrices (sf_potri_diag_batch): winv = sf_chol_inverse_work_doubles(n, batch) doubles of scratch,
// the strict upper triangle of L outside the 64 x 64 diagonal blocks is scratch too; arguments checked by the caller
size_t sf_chol_inverse_work_doubles(int n, int batch);
int sf_launch_chol_inverse_diag(double* L, int n, int lda, int64_t stride, int batch, double* winv, double* out,
                                int64_t out_stride, hipStream_t s);
// diag[batch][n] = the diagonals of the matrices
int sf_launch_diag_copy(const double* A, int n, int lda, int64_t stride, int batch, double* diag, hipStream_t s);

int sf_launch_clock_probe(long long* out, long long wall_ticks, hipStream_t s);

// sf_fill.hip (layers: sf_fill_elem.h, sf_fill_band.h, sf_fill_tile.h, sf_fill_dense.h, sf_fill_free.h, sf_cov_matvec.h, sf_cinv.h,
// sf_grad_frame.h, sf_cov_grad.h, sf_fisher_cov.h, sf_local_scan.h, sf_emu_grad.h)
struct sf_fill_args {
    const double* wave;    // [n]
    const double* sigma;   // [n]
    const double* Y;       // [B][mpad][ldy]  (rank-m factor rows, zero padded to mpad)
    const double* params;  // [B][pstride]
    double* C;             // [B] x stride
    int n, npad, lda, mpad, ldy, pstride;
    int64_t stride;
    int has_global, n_local, off_global, off_local;
    int lower_only;        // 1: only tiles touching the lower triangle, identity padding written
    int add_jitter;        // 1: + SF_JITTER on the diagonal
    int nout;              // rows / columns of C that are written; 0: npad with lower_only (workspace matrices: identity
                           // padding included), n otherwise.  Caller-owned matrices of n rows set it to n
    int monotonic;         // wave sorted ascending -> band culling allowed
    int loguniform;        // wave_i = wave_0 e^(i delta) to rounding -> K_global depends on i-j only
    unsigned char* tilemap; // optional [B][nt128*nt128]: 1 = the 128x128 tile is materialised in C
    int nt128;
    int fp;                // 0 or 64: the tile map / list index the tiles of the factorisation's shifted frame (sf_potrf_front_pad)
    // optional compact work list of the materialised tiles (likelihood path): k_tile_map appends (tm << 16 | tn) per flagged
    // 128 x 128 tile, the fill then launches a few workgroups per walker that walk the list instead of one (mostly empty)
    // workgroup per 64 x 64 tile of the whole matrix.  32-bit entries: nothing bounds N here, and 8-bit tile indices
    // would wrap at 256 tile rows (N > 32 768)
    unsigned* tilelist;        // [B][list_cap]
    int* tilecount;            // [B]
    int list_cap;
    double* gtab;          // optional [B][n] scratch: K_global per diagonal (log-uniform grids, likelihood path)
};
static inline __host__ __device__ int sf_fill_extent(const sf_fill_args& a) {
    return a.nout > 0 ? a.nout : (a.lower_only ? a.npad : a.n);
}
int sf_launch_fill(const sf_fill_args& a, int B, hipStream_t s);  // sf_fill_tile.h
// sf_fill_dense.h: dense (both triangles) matrices of the caller: plain / structured tiles split (smap, list: sf_fill_dense_map_tiles(n) per matrix)
size_t sf_fill_dense_map_tiles(int n);
// (ex: prepared executor whose auxiliary stream takes the structured tiles beside the plain ones, or NULL)
int sf_launch_fill_dense(const sf_fill_args& a, int B, unsigned char* smap, unsigned short* list, int* count, hipStream_t s,
                         sf_exec* ex);
int sf_launch_stream_write(double* dst, size_t count, double v, hipStream_t s);  // sf_fill_free.h
// sf_cov_matvec.h: out[b][k][r][0:n) = K_k v[b][r], k = emulator, noise (+ jitter), global, local 0 ... (3 + n_local
// components; zeros for a global kernel the model lacks; NaN where info[b] != 0).  f: fill_args (C unused); m rows of Y
// exist; v: [batch][nrhs][ldv]; yv: [batch][nrhs][m] scratch for Y v
int sf_launch_cov_matvec(const sf_fill_args& f, int m, const double* v, int ldv, int nrhs, int batch, double* yv,
                         const int* info, double* out, hipStream_t s);
// sf_cinv.h: selected 64 x 64 blocks of C^-1 = X^T X from what sf_launch_chol_inverse_diag leaves (X^T above the diagonal,
// winv); pairs: device [npairs][2] = (I, J), 0 <= J <= I < n / 64 (any other pair: a block of NaN); out: [batch][npairs][64][64]
int sf_launch_cinv_blocks(const double* L, int n, int lda, int64_t stride, int batch, const double* winv, const int* pairs,
                          int npairs, double* out, hipStream_t s);
// sf_cov_grad.h: the likelihood's gradient in the covariance hyper-parameters contracted from them (sf_grad_frame.h: the frame it
// shares with sf_emu_grad.h, the layout of part and the sum over the block rows): f as the fill gets it with C = the
// factored matrices after the inverse's launch; alpha: [batch][ld_alpha] = C^-1 r; part: sf_cov_grad_work_doubles of scratch;
// grad[b * grad_stride + slot]: log_amp, log_ls of the global kernel, then mu, log_amp, log_sigma per local kernel; NaN where
// info[b] != 0
static inline __host__ __device__ int sf_cov_grad_slots(int has_global, int n_local) { return (has_global ? 2 : 0) + 3 * n_local; }
size_t sf_cov_grad_work_doubles(int n, int has_global, int n_local, int batch);
int sf_launch_cov_grad(const sf_fill_args& f, int batch, const double* winv, const double* alpha, int ld_alpha, const int* info,
                       double* part, double* grad, int grad_stride, hipStream_t s);
// sf_fisher_cov.h: the Fisher information of the covariance hyper-parameters, F_ij = 1/2 tr(C^-1 dC_i C^-1 dC_j), in the slots
// of sf_launch_cov_grad: f, winv, info as sf_launch_cov_grad gets them; wf, tj: [batch][ld][ld] doubles of scratch each,
// ld = sf_fisher_cov_ld(n) (all of C^-1 and one T_j = C^-1 dC_j); part: sf_cov_grad_work_doubles of scratch;
// fisher[b * fisher_stride + i * slots + j], bit-symmetric, NaN where info[b] != 0
static inline __host__ __device__ int sf_fisher_cov_ld(int n) { return (n + SF_LEAF - 1) / SF_LEAF * SF_LEAF; }
int sf_launch_fisher_cov(const sf_fill_args& f, int batch, const double* winv, const int* info, double* wf, double* tj, double* part,
                         double* fisher, int fisher_stride, hipStream_t s);
// sf_local_scan.h: the score scan for a new local kernel at amplitude 0: f, winv, alpha, ld_alpha, info as sf_launch_cov_grad gets
// them on a monotonic grid; cand: [ncand][2] = mu, sigma (km/s), shared by the batch; patch: [ncand][2] ints and wband:
// sf_local_scan_band_doubles(n, batch) doubles of scratch (the patches; the block band of C^-1 with its mirror images);
// out[b][q][3] = alpha^T k alpha, tr(C^-1 k), 1/2 tr(C^-1 k C^-1 k): zeros for a candidate with no pixel in reach, NaN for one
// whose patch is wider than SF_LS_MAXP pixels and where info[b] != 0
size_t sf_local_scan_band_doubles(int n, int batch);
int sf_launch_local_scan(const sf_fill_args& f, int batch, const double* winv, const double* alpha, int ld_alpha, const int* info,
                         const double* cand, int ncand, int* patch, double* wband, double* out, hipStream_t s);
// sf_band_local_scan.h: the same scan from the band solver: sigma (lds doubles per row, ssigma per matrix) the band of Bd^-1 at
// the half-width wmax, vs[b * svs + c * ldv + i] the m columns of Vs (ldv >= n rounded up to whole 64-pixel blocks); wband:
// sf_local_scan_banded_doubles(n, batch) doubles; a patch wider than wmax + 1 pixels: NaN for every walker
size_t sf_local_scan_banded_doubles(int n, int batch);
int sf_launch_local_scan_banded(const sf_fill_args& f, int batch, const double* sigma, int lds, int64_t ssigma, int wmax,
                                const double* vs, int ldv, int64_t svs, int m, const double* alpha, int ld_alpha, const int* info,
                                const double* cand, int ncand, int* patch, double* wband, double* out, hipStream_t s);
// sf_grad_frame.h: the sum over the orders of a multi-order gradient (sf_multi_grad_reduce)
struct sf_multi_reduce_args {
    const double* unit_lnl;   // [nseg * W]
    const int* unit_info;     // [nseg * W]
    const double* unit_grad;  // [nseg * W][grad_stride]
    const int* col_ptr;       // [ncols + 1]
    const int* col_src;       // [col_ptr[ncols]][2]: (segment, slot)
    int nseg, W, grad_stride, ncols, out_stride;
    double* lnl;   // [W]
    double* grad;  // [W][out_stride]
    int* info;     // [W]
};
int sf_launch_multi_grad_reduce(const sf_multi_reduce_args& a, hipStream_t s);
// sf_emu_grad.h: the emulator training likelihood's gradient in the LOGS of its hyper-parameters, contracted from the blocks of
// v11^-1: grid, hyper (raw rows), iphiphi as sf_launch_v11_build_batch gets them; L: the factored matrices after the inverse's
// launch; alpha: [batch][ld_alpha] = v11^-1 w_hat; part: sf_emu_grad_work_doubles of scratch; grad[b * grad_stride + slot] in
// the order of the raw row; NaN where info[b] != 0
static inline __host__ __device__ int sf_emu_grad_slots(int m, int P) { return 1 + m + m * P; }
size_t sf_emu_grad_work_doubles(int M, int P, int m, int batch);
int sf_launch_emu_grad(const double* grid, int M, int P, int m, const double* hyper, int hyper_stride, int batch,
                       const double* iphiphi, const double* L, int npad, int lda, int64_t stride, const double* winv,
                       const double* alpha, int ld_alpha, const int* info, double* part, double* grad, int grad_stride,
                       hipStream_t s);
// sf_fill_band.h: band storage of the structured part of C (sf_band.hip consumes it); a.npad = rows written (>= a.n)
int sf_launch_band_fill(const sf_fill_args& a, int B, double* band, int ws, int halfwidth, int ldb, int64_t sband,
                        int* info, double* gtab, hipStream_t s, int tile_wt = -1);  // ws stored diagonals > halfwidth; gtab: B x (ws+1) or NULL
int sf_launch_global_cov(const double* wave, int n, double amp, double ls, double* out, hipStream_t s);  // sf_fill_free.h
int sf_launch_local_cov(const double* wave, int n, double amp, double mu, double sigma, int accumulate,
                        double* out, hipStream_t s);

// sf_band.hip (layers: sf_band_shape.h, sf_band_window.h, sf_band_sweep.h, sf_band_twist.h, sf_band_woodbury.h, sf_band_solve.h, sf_band_selinv.h, sf_band_diag.h): banded
// Cholesky + forward substitution of (1 + m) right-hand sides -> logdet, Gram matrix
// The right-hand sides of a batch: row r of matrix b at rhs + b * srhs + r * ldr.  Optional separate source for row 0 (the
// residual lives in its own buffer in the fused path): when rhs0 is given, rows 1.. come from rhs rows 0..
struct sf_band_rhs {
    const double* rhs;
    int64_t srhs;
    int ldr, nrhs;
    const double* rhs0;
    int64_t srhs0;
    __device__ sf_band_rhs of(int b) const {  // matrix b alone, as a batch of one
        return sf_band_rhs{rhs + (int64_t)b * srhs, 0, ldr, nrhs, rhs0 ? rhs0 + (int64_t)b * srhs0 : nullptr, 0};
    }
    __device__ const double* row(int r) const {  // row r of the first matrix
        return rhs0 ? (r == 0 ? rhs0 : rhs + (int64_t)(r - 1) * ldr) : rhs + (int64_t)r * ldr;
    }
};
// One call of the band solver: the band view (band[i*ldb + d] = A[i][i-d], d in [0, halfwidth], matrices sband apart), the
// order and the batch, the right-hand sides; outputs logdet [batch], gram [batch][nrhs*nrhs], info [batch] (first
// non-positive pivot, 1-based; left untouched otherwise)
struct sf_band_call {
    const double* band;
    int64_t sband;
    int ldb, halfwidth, n, batch;
    sf_band_rhs r;
    double *logdet, *gram;
    int* info;
};
int sf_launch_band_forms(const sf_band_call& c, hipStream_t s);
// two half sweeps + separator (halves the sequential chain when 2*batch workgroups fit the chip); work: sfb_twist_carve
bool sf_band_twisted_applicable(int n, int halfwidth, int batch);
int sf_launch_band_forms_twisted(const sf_band_call& c, double* work, hipStream_t s);
int sf_launch_woodbury(const double* gram, int nrhs, int batch, const double* logdet_band, double* logdet,
                       double* sqmah, int* info, hipStream_t s);
// sf_band_solve.h: the full solve on the LDS window (sfb_admit(...) == SFB_WINDOW only).  The keeping sweep is
// sf_launch_band_forms' single sweep, which also stores the factor and the forward-substituted right-hand sides in fac
// (sfb_keep_doubles(n, nbr, nrb) doubles per matrix); the backward sweep turns them into x[b * sx + r * ldx + i] = (A^-1 rhs_r)_i
// (NaN where info[b] != 0); the mix forms [alpha, V] = C^-1 [R^T, X^T] = T M in the staging layout [batch][kr + nv][npad] from
// T = Bd^-1 [R^T, Y^T] ([batch][kr + m][npad]: kr right-hand sides in front of Y; the mean gradient's residual is kr = 1), the
// sweep's Gram matrix and Lw (nv = m: with V; nv = 0: alpha alone, Lw not read).  Mwork: [batch][(kr + m)(kr + nv)]; flag: NULL,
// or the walkers' status, which a non-positive pivot of the capacitance matrix sets to SF_INFO_BAD_WEIGHT_COV
int sf_launch_band_keep(const sf_band_call& c, double* fac, hipStream_t s);
int sf_launch_band_back(const double* fac, int n, int halfwidth, int batch, int nrhs, const int* info, double* x, int ldx, int64_t sx,
                        hipStream_t s);
int sf_launch_band_mix(const double* gram, const double* Lw, int kr, int m, int nv, const int* info, int* flag, const double* T, int n,
                       int npad, int batch, double* Mwork, double* stage, hipStream_t s);
// sf_band_selinv.h: the band of Sigma = A^-1 from the records of sf_launch_band_keep (same n, halfwidth, nrhs), by selected
// inversion: out[b * sout + i * ldo + d] = Sigma[i][i - d], 0 <= d <= min(i, halfwidth), i < n (NaN where info[b] != 0); and
// Vs = T_Y L_S^-T of C^-1 = Sigma - Vs Vs^T in rows co .. co + m - 1 of stage2 ([batch][co + m][npad]; co = kr = 1: the staging
// layout of the gradient's sf_launch_band_mix, row 0 zero; co = 0: the m columns alone), Mwork: [batch][(kr + m)(co + m)]
int sf_launch_band_selinv(const double* fac, int n, int halfwidth, int batch, int nrhs, const int* info, double* out, int ldo,
                          int64_t sout, hipStream_t s);
int sf_launch_band_vs(const double* gram, int kr, int m, int co, const int* info, const double* T, int n, int npad, int batch,
                      double* Mwork, double* stage2, hipStream_t s);
// sf_band_diag.h: what the diagnostics on the band solver add.  The rows [R; Y] of a sweep with caller right-hand sides:
// buf[b][r] = rhs[b * rhs_stride + r * ldr + 0:n) padded with zeros to npad for r < kr, then the m rows of Y
// (Y[b * sy + j * npad + 0:npad)).  cinv_diag[b][i] = sigma[b * ssigma + i * lds] - sum_c vs[b * svs + c * ldv + i]^2, c
// ascending; cov_diag[b][i] = band[b * sband + i * ldb] + sum_j Y[b * sy + j * ldy + i]^2, j ascending: the diagonal of
// C = Bd + Y^T Y as it is factorised; both [batch][n], NaN where info[b] != 0
int sf_launch_band_diag_stage(const double* rhs, int ldr, int64_t rhs_stride, const double* Y, int64_t sy, int n, int npad, int kr,
                              int m, int batch, double* buf, hipStream_t s);
int sf_launch_band_cinv_diag(const double* sigma, int lds, int64_t ssigma, const double* vs, int ldv, int64_t svs, int m,
                             const int* info, int n, int batch, double* cinv_diag, hipStream_t s);
int sf_launch_band_cov_diag(const double* band, int ldb, int64_t sband, const double* Y, int ldy, int64_t sy, int m, const int* info,
                            int n, int batch, double* cov_diag, hipStream_t s);
// sf_fill.hip (sf_band_cov_grad.h): the covariance gradient contracted over the band, slots and part as sf_launch_cov_grad;
// sigma: the band of Bd^-1 (lds doubles per row, ssigma per matrix); alpha[b * sstage + i]; vs[b * sstage + c * ldv + i], c < m
int sf_launch_band_cov_grad(const sf_fill_args& f, int batch, const double* sigma, int lds, int64_t ssigma, int halfwidth,
                            const double* alpha, const double* vs, int ldv, int64_t sstage, int m, const int* info, double* part,
                            double* grad, int grad_stride, hipStream_t s);
// sf_chol.hip (sf_chol_band.h): wide bands (beyond the LDS window) as bordered band matrices on the fused panel kernel;
// c.band is not read: the tiles hold the matrix, nband rows of it
int sf_launch_potrf_band(const sf_band_call& c, int nband, double* tiles, hipStream_t s);
