// Host-side launch API for every hand-written gfx950 kernel in csrc/kernels.
// All launchers are asynchronous on the given stream and graph-capturable
// (no allocation, no synchronisation inside).
#pragma once
#include <vector>

#include <hip/hip_runtime.h>

#include <cstdint>

namespace atpu {

typedef __bf16 bf16;

// ---------------------------------------------------------------- random init (atpu/rand.h)
// dst[i] = Irwin-Hall(4) value of (seed, sid, i) x (i < n0 ? scale0 : scale1), bf16 (RNE) or fp32;
// bit-identical to rand_fill_host (runtime.h)
void rand_fill(void* dst, int64_t n, bool f32, uint64_t seed, uint64_t sid, float scale0, int64_t n0, float scale1,
               hipStream_t stream);

// ---------------------------------------------------------------- GEMM (K3/K5/K6)
enum GemmEpilogue : int {
  kEpiBias = 1,
  kEpiGelu = 2,
  kEpiTanh = 4,
  kEpiResidual = 8,
  kEpiRelu = 16,
  kEpiOutF32 = 32,  // C is float* (128x128 kernel only; LM-head logits)
  // LayerNorm folding (post-LN encoders; persistent 256x256 full-line kernel only,
  // M, N, K multiples of 256). LN(x) = (x - mu) * rstd * gamma + beta is never
  // materialised: its producer emits row statistics, its consumers apply them.
  kEpiInNorm = 64,     // A rows are raw LN inputs, gamma folded into Bt, beta into bias:
                       //   C = rstd*acc - rstd*mu*colsum + bias    (rstd, mu from in_fin)
  kEpiResNorm = 128,   // R rows are raw LN inputs (beta folded into bias):
                       //   C = ... + (R*rstd - rstd*mu) * gamma     (rstd, mu from res_fin)
  kEpiStatsOut = 256,  // also write per-row partial (sum, sum of squares) of C, one per 256 columns
  kEpiKvScatter = 1024,  // decode QKV: columns >= kv_col0 (K|V) go to the KV cache at row m*kv_T + *kv_step
                         //   (leading dim kv_ld), columns < kv_col0 (Q) to C (128x128 / "dec" kernels)
  kEpiRowRms = 512,    // A rows are raw RMSNorm inputs (gamma folded into Bt): the kernel sums A^2
                       //   over its K loop, C = rsqrt(mean_k A^2 + rms_eps) * (A . Bt^T) ... (128x128 and
                       //   skinny "dec" kernels, no split-K; T5 decoder steps)
  // LayerNorm folding for decode steps (post-LN decoders, BART; 128x128 and "dec" kernels,
  // no split-K). Row statistics travel as partial (sum, sumsq) per 32-column slab:
  kEpiRowLn = 2048,     // A rows are raw LN inputs, gamma folded into Bt, beta into bias:
                        //   C = rstd*acc - rstd*mu*colsum + bias, (mu, rstd) of A's rows from in_part
                        //   [K/32][M][2] (eps in rms_eps)
  kEpiResLn = 4096,     // R rows are raw LN inputs (beta folded into bias), stats from res_part
                        //   [N/32][M][2]: C = ... + (R*rstd - rstd*mu) * gamma
  kEpiRowStats = 8192,  // also write part_out [N/32][M][2]: (sum, sumsq) of the bf16-rounded C
                        //   values of each row's 32-column slabs
};

// GemmArgs::layout bits
constexpr int kLayA = 1, kLayC = 2, kLayR = 4;
// fragment order (set WITH the operand's image bit, = that bit << 3): the 16-byte units inside
// each image re-ordered so that one lane's packed accumulator fragment is a unit
constexpr int kLayFragA = 8, kLayFragC = 16, kLayFragR = 32;
static_assert(kLayFragA == kLayA << 3 && kLayFragC == kLayC << 3 && kLayFragR == kLayR << 3, "frag bit = image bit << 3");

struct GemmArgs {
  const bf16* A = nullptr;  // [M, K] row-major, leading dim lda
  int lda = 0;
  const bf16* Bt = nullptr;  // [N, K] row-major (nn.Linear.weight layout)
  int ldb = 0;
  bf16* C = nullptr;  // [M, N], leading dim ldc
  int ldc = 0;
  const float* bias = nullptr;  // [N] fp32
  const bf16* R = nullptr;      // residual [M, N], leading dim ldr
  int ldr = 0;
  int M = 0, N = 0, K = 0;
  int epi = 0;
  // operand layout (kLayA | kLayC | kLayR): the operand [M, W] lies in K-tile image order
  // [M/256][W/64][256][64] (element (r, c) at (((r/256)*(W/64) + c/64)*256 + r%256)*64 + c%64)
  // with W = its leading dimension; one image is a K-tile of the consuming 256x256 GEMM's A
  // operand and the 64 columns one wave of the producing GEMM writes. 0 = row-major.
  // Persistent full-line 256x256 kernel (M, N % 256 == 0) and the fused QKV + attention
  // kernel (A, and C = the context: head h of a 2-sequence tile is image h of its row tile).
  // Fragment order (kLayFragA / C / R with the image bit; A of both kernels, C and R of the GEMM):
  // same images, inside one [16 row groups of 16 rows][2 k-halves of 32 columns][64 units of
  // 16 B]; unit u = row u % 16 of the group, columns ([0,2,1,3][u / 16]) * 8 .. + 7 of the half:
  // what lane u holds after v_permlane16_swap of its packed fragments (j0, j1) or (j2, j3). The
  // producer stores it without an LDS transpose, the consumer's LDS image is a verbatim copy.
  int layout = 0;
  // split-K (skinny M): splits > 1 needs ws = fp32 [splits, M, N]
  int splits = 1;
  float* ws = nullptr;
  // LayerNorm folding (see kEpiInNorm / kEpiResNorm / kEpiStatsOut)
  const float* in_fin = nullptr;   // InNorm: [M][2] (rstd, rstd*mu) of A's rows
  const float* colsum = nullptr;   // InNorm: [N] fp32, colsum[n] = sum_k Bt[n][k]
  const float* res_fin = nullptr;  // ResNorm: [M][2] (rstd, rstd*mu) of R's rows
  const float* gamma = nullptr;    // ResNorm: [N] LN gamma of R
  float* part_out = nullptr;       // StatsOut: [N/256][M][2] partial (sum, sumsq) of C's rows (fp32 values)
  const float* in_part = nullptr;   // RowLn: [K/32][M][2] (sum, sumsq) partials of A's rows (+ colsum)
  const float* res_part = nullptr;  // ResLn: [N/32][M][2] partials of R's rows (+ gamma); RowStats: part_out
  float rms_eps = 0.f;             // RowRms
  bf16* kv_cache = nullptr;        // KvScatter: cache [rows * kv_T, kv_ld]
  int kv_ld = 0, kv_T = 0, kv_col0 = 0;
  const int32_t* kv_step = nullptr;  // device scalar: the position being written
  // GEMV (<= 4 rows) only: the weight [pf_n, pf_k] (row stride pf_ld) of the NEXT GEMV of a
  // decode chain, pulled into the L2 of the XCD that will read it (ATPU_GEMV_PREFETCH)
  const bf16* pf_w = nullptr;
  int pf_ld = 0, pf_k = 0, pf_n = 0;
  int pf_rpb = 16;  // weight rows per workgroup of that next GEMV (32 when it writes RowStats)
};
void gemm_bf16(const GemmArgs& g, hipStream_t stream);
// true when gemm_bf16 runs an [M, N] problem with epilogue `epi` on the <= 4-row GEMV (the
// same test it applies: ATPU_GEMV, ATPU_GEMM_TILE, N % 16, an instantiated epilogue)
bool gemv_selected(int M, int N, int epi);
// split count the library picks for an [M,N,K] problem (1 = no split-K)
int gemm_splitk_splits(int M, int N, int K);
// skinny-M selector (benchmarks): 1 = 64x64 multi-stage dec kernel, 0 = 128x128 split-K
int gemm_dec_mode(int set);
// batch-invariant kernel selection (ATPU_BATCH_INVARIANT): no GEMV / split-K GEMMs, no split
// cross attention / few-row self attention, no few-row LM head or merge; set 0/1, -1 reads
int batch_invariant(int set);
// kernel family override (benchmarks/tests): 0 auto, 64 dec, 128, 256; -1 reads
int gemm_force_tile(int set);
// 256x256 schedule selector (benchmarks): set >= 0 switches; returns the current
int gemm_256_variant(int set);
// persistent 256 x 192 GEMM (qkv_attn.hip; one BERT head's Q|K|V per tile): epi = Bias or
// Bias|InNorm; mode 0 stores C, 1 = timing only (no epilogue, C untouched)
void gemm256h(const GemmArgs& g, int mode, hipStream_t stream);
// BERT QKV projection + self-attention in one persistent kernel (S = 128, head dim 64):
// Bt = the QKV weight with rows in [head][Q 64 | K 64 | V 64] order (bias / colsum likewise),
// g.C = the context [M, N / 3] (row stride g.ldc), lens[M / 128] the sequence lengths
void qkv_attention(const GemmArgs& g, const int32_t* lens, float scale, hipStream_t stream);
// [CLS] attention of the last BERT layer without a K / V projection (cls_attend.hip): g [B*128, H]
// raw hidden rows, fin [B*128, 2] their (rstd, rstd*mu), U [B, heads*H] one projected query per
// head, Z [B, heads*H] = sum_j p_hj LN0(g_j) (LN0: no gamma / beta). S = 128, H % 256 == 0,
// H <= 1024, heads = H / 64 <= 16; lens clamped to [1, 128]
void cls_attend(const bf16* g, const float* fin, const bf16* U, const int32_t* lens, bf16* Z, int B, int S, int H,
                int heads, hipStream_t stream);
// Sentence embedding (pool_embed.hip): out [B, H] fp32 = the mean over the rows j < len (mode
// kPoolMean) or row 0 (kPoolCls) of x [B*S, H]. With fin [B*S, 2] = (rstd, rstd*mu), x holds raw
// rows and the LayerNorm (gamma, beta, both required) is applied to the pooled vector; with
// fin == nullptr x is already normalised (gamma / beta unused). normalize != 0: out divided by
// max(||out||_2, 1e-12). S in [1, 512], H % 64 == 0, H in [64, 1024]; lens clamped to [1, S]
enum PoolMode : int { kPoolMean = 0, kPoolCls = 1 };
void pool_embed(const bf16* x, const float* fin, const float* gamma, const float* beta, const int32_t* lens,
                float* out, int B, int S, int H, int mode, int normalize, hipStream_t stream);
// Top-k similarity search (sim_topk.hip): scores = q [nq, D] . c [N, D]^T in exact fp32 (one
// k-ordered fmaf chain per pair, the order a function of D alone), the [nq, N] matrix never
// written. sim_topk_partial leaves every split's sorted top-k (value, row as int bits) in
// ws [nq, P, k, 2] fp32; sim_topk_merge reduces it to scores [nq, kk] / ids [nq, kk] =
// id_base + row, ordered by (value desc, row asc). D % 64 == 0, D in [64, 1024], k in [1, 32],
// kk = min(k, N), N < 2^31 - 256. P = sim_topk_splits(N, wanted) <= kSimMaxSplits (no empty split).
// Nothing outside c[0:N] is read.
constexpr int kSimMaxSplits = 256;
int sim_topk_splits(int N, int want);
void sim_topk_partial(const float* q, const float* c, float* ws, int nq, int N, int D, int k, int P,
                      hipStream_t stream);
void sim_topk_merge(const float* ws, float* scores, int64_t* ids, int nq, int P, int k, int kk, int64_t id_base,
                    hipStream_t stream);
// The same over a float16 corpus c [N, D] (sim_topk_f16.hip): every score is the exact fp32 dot
// product of q and the widened stored values, times row_scale[row] (fp32 [N], or nullptr) before
// the ranking. Same shapes, workspace and merge; its k order is its own (a function of D alone).
// Nothing outside c[0:N] and row_scale[0:N] is read.
void sim_topk_partial_f16(const float* q, const _Float16* c, const float* row_scale, float* ws, int nq, int N, int D,
                          int k, int P, hipStream_t stream);
// Filtered forms (sim_topk_masked.hip): only the rows whose bit is set in words [ceil(N / 32)] int32
// (bit b of word w = row 32 w + b; bits at or past N are ignored) enter the lists; live [n_live]
// int32 lists the non-zero words in ascending order, and only those 32-row steps are read. A score
// has the bits of the unmasked kernel for the same (q, row), so the result equals sim_topk over the
// gathered allowed rows with the ids mapped back. P = sim_topk_splits_live(n_live, wanted); the
// workspace and sim_topk_merge are the same (kk <= the count of allowed rows is the caller's).
// Nothing outside c[0:N], row_scale[0:N], words[0:ceil(N/32)] and live[0:n_live] is read.
int sim_topk_splits_live(int n_live, int want);
void sim_topk_partial_masked(const float* q, const float* c, const int32_t* words, const int32_t* live, float* ws,
                             int nq, int N, int D, int k, int P, int n_live, hipStream_t stream);
void sim_topk_partial_masked_f16(const float* q, const _Float16* c, const float* row_scale, const int32_t* words,
                                 const int32_t* live, float* ws, int nq, int N, int D, int k, int P, int n_live,
                                 hipStream_t stream);
// Row-mask builders (sim_topk_masked.hip): words [ceil(N / 32)] and *count (int64, the set bits) are
// written whole. from_ids: the bit of every id in [base, base + N) (duplicates and other ids are
// harmless); exclude inverts, with the tail bits at or past N cleared. from_labels: rows whose label
// is one of values [m <= kRowMaskMaxValues] (sorted ascending), or with values == nullptr in [lo, hi].
constexpr int kRowMaskMaxValues = 256;
void row_mask_from_ids(const int64_t* ids, int64_t m, int64_t base, int N, int exclude, int32_t* words,
                       int64_t* count, hipStream_t stream);
void row_mask_from_labels(const int64_t* labels, int N, const int64_t* values, int m, int64_t lo, int64_t hi,
                          int32_t* words, int64_t* count, hipStream_t stream);
// IVF form (sim_topk_ivf.hip): the corpus sorted by cluster, vectors [N, D] fp32 with row_ids [N] int32 (the
// original row of a sorted row) and offsets [K + 1] int32; every query searches the clusters of its own
// nprobe probe slots. The plan groups the nq * nprobe (query, slot) pairs by cluster into `items` work items
// of at most kIvfItemQueries queries of one cluster: item_cluster [items] (negative: a surplus item),
// item_query / item_slot [items, 16] (negative slot: padding, its query a valid one). One workgroup per
// (item, split of S) leaves the sorted top-k (value, ORIGINAL row) of (query, slot, split) in
// ws [nq, nprobe * S, k, 2] fp32, every slot written, for sim_topk_merge with P = nprobe * S <= kSimMaxSplits.
// A score has sim_topk's bits for the same (q, row). K in [1, 4096], nprobe in [1, min(32, K)];
// items <= sim_topk_ivf_items(nq, nprobe, K) = min(nq * nprobe, K) + nq * nprobe / 16, the bound to launch.
// Nothing outside q, vectors[0:N], row_ids[0:N], offsets[0:K + 1] and the plan arrays is read.
constexpr int kIvfItemQueries = 16;
int64_t sim_topk_ivf_items(int64_t nq, int nprobe, int K);
// The plan of probes [nq, nprobe] int64 (cluster ids in [0, K); others are skipped) in one launch: the three plan
// arrays written whole, items == sim_topk_ivf_items(nq, nprobe, K). Every pair lands in exactly one item.
void sim_topk_ivf_plan(const int64_t* probes, int nq, int nprobe, int K, int items, int32_t* item_cluster,
                       int32_t* item_query, int32_t* item_slot, hipStream_t stream);
void sim_topk_ivf_partial(const float* q, const float* vectors, const int32_t* row_ids, const int32_t* offsets,
                          const int32_t* item_cluster, const int32_t* item_query, const int32_t* item_slot, float* ws,
                          int nq, int N, int D, int k, int K, int nprobe, int S, int items, hipStream_t stream);

// ---------------------------------------------------------------- product quantization (pq.hip)
// A row of D floats as M bytes: byte m = the codeword (of 256) of sub-space m, columns m * dsub .. + dsub - 1.
// dsub = D / M in {4, 8, 16}, M a multiple of 4 in [4, kPqMaxSubvectors]. A sub-space dot product is the chain
// p_0, + p_1, ... of separately rounded products (no FMA), in all three kernels.
// pq_encode: codes[i, m] = arg-max over j of dot(x[i, sub m], codebooks[m, j]) + bias[m, j] (one fp32 add), ties
// to the lower j (+0.0 and -0.0 tie); x [n, D], codebooks [M, 256, dsub], bias [M, 256], codes [n, M] row-major.
// pq_lut: lut[i, m, j] = dot(q[i, sub m], codebooks[m, j]); lut [nq, M, 256].
// pq_scan_partial: score(i, r) = lut[i, 0, code(r, 0)] + lut[i, 1, code(r, 1)] + ... in ascending m, one fp32
// chain; every split's sorted top-k (value, row as int bits) goes to ws [nq, P, k, 2] for sim_topk_merge,
// P = pq_scan_splits(N, wanted) <= kSimMaxSplits (no empty split). codes is the interleaved layout
// [ceil(N / 64)][M / 4][64][4] bytes: byte e of dword (b, m4, lane) = code(64 b + lane, 4 m4 + e), the rows past N
// of the last block present (any value). k in [1, 32], N < 2^31 - 256. Nothing outside these tensors is read.
constexpr int kPqMaxSubvectors = 128;
bool pq_shape_ok(int D, int M);
void pq_encode(const float* x, const float* codebooks, const float* bias, uint8_t* codes, int64_t n, int D, int M,
               hipStream_t stream);
void pq_lut(const float* q, const float* codebooks, float* lut, int nq, int D, int M, hipStream_t stream);
int pq_scan_splits(int N, int want);
void pq_scan_partial(const float* lut, const uint8_t* codes, float* ws, int nq, int N, int M, int k, int P,
                     hipStream_t stream);

// ---------------------------------------------------------------- k-means (kmeans.hip)
// Assignment step: labels[i] = arg-max over k of dot(x[i], c[k]) (+ bias[k], one fp32 add; nullptr = none)
// in the order of better() (score desc, centroid asc), best[i] that score; every score is one fp32
// accumulator fed in sim_topk's column order, so without a bias (labels, best) equal sim_topk(x, c, 1)
// bit for bit, whatever the launch shape. *changed (int64, zeroed here) counts labels[i] != prev_labels[i].
// D % 64 == 0, D in [64, 1024], K in [1, kKmeansMaxK], N in [1, 2^31 - 256]. max_wgs: a cap on the
// persistent grid (0: the device's own), for tests. Nothing outside the tensors is read.
constexpr int kKmeansMaxK = 4096;
bool kmeans_shape_ok(int D, int K);
void kmeans_assign(const float* x, const float* c, const float* bias, const int32_t* prev_labels, int32_t* labels,
                   float* best, int64_t* changed, int N, int K, int D, int max_wgs, hipStream_t stream);
// Order-free sum: *out = sum_i rint(v[i] * 2^shift) as int64 (ties to even; integer adds, any order).
void fixed_sum(const float* v, int64_t n, int shift, int64_t* out, hipStream_t stream);
// Centroid update: sums[k, d] = sum over labels[i] == k of rint(x[i, d] * 2^shift), counts[k] = members
// (both int64, zeroed here; a label outside [0, K) leaves its row out). ws: kmeans_update_ws_bytes(N, K).
size_t kmeans_update_ws_bytes(int N, int K);
void kmeans_update(const float* x, const int32_t* labels, int shift, int64_t* sums, int64_t* counts, int32_t* ws,
                   int N, int K, int D, hipStream_t stream);
// New centroids: for counts[k] > 0 the mean float(double(sum) / (double(count) * 2^shift)), divided by
// max(its fp64 norm, 1e-12) when cosine; an empty cluster keeps c_old[k]. bias (or nullptr)
// = float(-0.5 * ||c_new[k]||^2). fp64, one rounding per operation, columns ascending. c_new may be c_old.
void kmeans_finalize(const int64_t* sums, const int64_t* counts, const float* c_old, float* c_new, float* bias, int K,
                     int D, int shift, int cosine, hipStream_t stream);

// ---------------------------------------------------------------- near-duplicates (sim_join.hip)
// Similarity join: every pair (I, J) = (x_base + i, y_base + j) with I < J and dot(x[i], y[j]) >= threshold
// (an fp32 compare; the score is one fp32 accumulator fed in sim_topk's column order, so it has sim_topk's
// bits whatever the launch shape) goes to pairs [cap, 2] / scores [cap] in arbitrary order. *count (int64,
// zeroed here) ends as the true total, also beyond cap; nothing is written at or past cap. D % 64 == 0,
// D in [64, 1024]; every id in [0, 2^31 - 256). max_wgs caps the persistent grid and panel_steps sets the
// 32-row steps of y per work item (0: the defaults); the emitted set depends on neither. Nothing outside
// x[0:Nx] and y[0:Ny] is read.
bool sim_join_ok(int D);
void sim_join(const float* x, const float* y, float threshold, int Nx, int Ny, int D, int x_base, int y_base,
              int32_t* pairs, float* scores, int64_t* count, int64_t cap, int max_wgs, int panel_steps,
              hipStream_t stream);
// Connected components by minimum label: cc_init sets parent[v] = v; cc_round hooks every edge of
// pairs [E, 2] (atomicMin, parent[v] <= v always) and compresses every node to its root, and leaves
// *changed (int32, zeroed here) != 0 when a hook lowered a parent. The caller repeats rounds until one
// changes nothing; parent then holds every node's smallest component member. Edges with an endpoint
// outside [0, N) are skipped.
void cc_init(int32_t* parent, int N, hipStream_t stream);
void cc_round(const int32_t* pairs, int64_t E, int32_t* parent, int N, int32_t* changed, hipStream_t stream);

// ---------------------------------------------------------------- INT8 GEMM (gemm_i8.hip)
// Symmetric per-row quantisation, 127 levels: scale[r] = amax_r / 127 (1 for an all-zero row),
// q[r][k] = clamp(rint(x[r][k] * (127 / amax_r)), -127, 127). One wave per row; K % 16 == 0,
// 16-B aligned x rows, 8-B aligned q rows. Weights [N, K] go through the same kernel (per
// output channel). Inf / NaN inputs are unspecified.
void quantize_rows_i8(const bf16* x, int ldx, int8_t* q, int ldq, float* scale, int rows, int K,
                      hipStream_t stream);
struct GemmI8Args {
  const int8_t* A = nullptr;  // [M, K] row-major, leading dim lda (bytes)
  int lda = 0;
  const float* a_scale = nullptr;  // [M]
  const int8_t* Bt = nullptr;      // [N, K] row-major
  int ldb = 0;
  const float* b_scale = nullptr;  // [N]
  bf16* C = nullptr;               // [M, N], leading dim ldc
  int ldc = 0;
  const float* bias = nullptr;  // [N] fp32
  const bf16* R = nullptr;      // residual [M, N], leading dim ldr
  int ldr = 0;
  int M = 0, N = 0, K = 0;
  int epi = 0;  // kEpiBias | kEpiGelu | kEpiResidual
  // when set: write the raw int32 accumulators [M, N] (leading dim ldacc) and nothing else
  int32_t* acc_out = nullptr;
  int ldacc = 0;
};
// C = bf16(gelu?(float(A . Bt^T) * a_scale[m] * b_scale[n] + bias[n]) + R[m][n]), int32 accumulation
// on v_mfma_i32_16x16x64_i8 (exact). One 128x128 kernel for every M, no split-K: a row's result
// does not depend on M or on the tile it lands in.
void gemm_i8(const GemmI8Args& g, hipStream_t stream);
// shapes gemm_i8 takes: M >= 1, N % 16 == 0, K % 64 == 0, K <= 2^17
bool gemm_i8_ok(int M, int N, int K);
// layernorm_bf16 with a second output: the bf16 row and its quantisation (q, scale), bit for
// bit quantize_rows_i8 of the bf16 output, in one pass over the row
void layernorm_quant_i8(const bf16* x, const bf16* res, const float* gamma, const float* beta, bf16* out, int8_t* q,
                        float* scale, int rows, int N, float eps, hipStream_t stream);

int attention_persist_mode(int set);  // packed BERT attention: 1 persistent (default), 0 per-item
int num_cus();                        // CUs a persistent grid is sized for (device count, or the budget below)
int cu_budget(int set);               // >0: size persistent grids for this many CUs (CU-masked streams)
int64_t make_cu_mask_stream(int first_bit, int nbits);  // hipStream_t over CU-mask bits [first, first+n)

// ------------------------------------------------------------ decode (K9-K11)
// One query row per (row, head) against a KV cache. Cross attention (lens set):
// key j of row r lives at k/v + ((r / group) * seq_stride + j) * ldkv + h*64,
// length lens[r / group]; one workgroup serves the `group` rows of a sequence.
// Self attention (step_dev set, group 1): length *step_dev + 1; key j < len-1
// of row r lives in physical row hist[r * hist_stride + j] when hist is given
// (beam backpointers), else in row r. bias_dist (fp32 [H, bias_stride]) adds
// bias_dist[h][len-1-j] (T5 decoder relative position bias).
void decode_attention(const bf16* q, int ldq, const bf16* k, const bf16* v, int ldkv, int seq_stride, int group,
                      const int32_t* lens, const int32_t* step_dev, const int32_t* hist, int hist_stride,
                      const float* bias_dist, int bias_stride, bf16* out, int ldo, int rows, int H, float scale,
                      hipStream_t stream, float* ws = nullptr);
// Cross attention (lens) over a grid of few items splits the keys into 64-key chunks
// (flash decoding) when given a workspace of this many floats (0: no split for the shape).
int decode_attention_splits(int rows, int group, int H, int seq_stride, bool cross);
size_t decode_attention_ws_floats(int rows, int group, int H, int seq_stride, bool cross);
int decode_self_few(int set);  // 1: few-row self attention one wave per (row, head), T <= 192 (default); -1 reads
// one-workgroup state advance of a small beam search (rows x stride x 4 B x (seq ? 2 : 1) <= 64 KiB):
// hist / seq reordered in place by par (as beam_reorder_hist, seq with last = tok, off 1),
// tokens = tok, *step_dev += 1
size_t decode_advance_lds(int rows, int stride, bool seq);
// decoder input of the new tokens, written by decode_advance (table == nullptr: none):
// out[r] = table[tok[r]], or with gamma LN(table[tok[r]] + pos[step + 1 + pos_off])
struct DecEmbed {
  const bf16* table = nullptr;
  int vocab = 0;
  const bf16* pos = nullptr;
  int pos_off = 0, npos = 0;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  float eps = 0.f;
  bf16* out = nullptr;
};
void decode_advance(int32_t* hist, int32_t* seq, int rows, int stride, const int32_t* par, const int32_t* tok,
                    int32_t* tokens, int32_t* step_dev, hipStream_t stream, const DecEmbed& em = DecEmbed{},
                    int N = 0);
// dst[r][j] = src[parent[r]][j] (j < t), dst[r][t] = last ? last[r] : parent[r]; t = *step_dev + off
// device beam selection (runtime/summarize.py): item top-K2 over its beams' candidates, hits,
// next running beams -> stage [parents | tokens | score bits] and a host record per item
// device address of a pinned host buffer of `bytes` (checked with hipPointerGetAttributes)
uintptr_t host_device_ptr(uintptr_t host, size_t bytes);
void beam_select(const float* sc, const int32_t* tk, int B, int nb, int K2, int V, int eos, int hit_all, float neg,
                 int32_t* stage, int32_t* rec, hipStream_t stream);
void beam_reorder_hist(const int32_t* src, int32_t* dst, const int32_t* parent, int rows, int stride,
                       const int32_t* step_dev, hipStream_t stream, const int32_t* last = nullptr, int off = 0);
void kv_append(const bf16* src, int lds, int col0, int ncols, bf16* cache, int seq_stride, int ldc,
               const int32_t* step_dev, int rows, hipStream_t stream);
void gather_rows(const bf16* src, bf16* dst, const int32_t* parent, int nrows, int seq_stride, int ldc,
                 const int32_t* step_dev, int slabs, size_t slab_elems, hipStream_t stream);
void beam_topk_rows(const float* logits, int rows, int V, const float* beam_scores, int eos, int mask_eos, int K,
                    float* out_score, int32_t* out_token, hipStream_t stream,
                    const int32_t* bans = nullptr, int nbmax = 0, const int32_t* seq = nullptr, int seq_stride = 0,
                    int cur = 0, int ngram = 0);
// Fused LM head + beam top-k (lm_head.hip): the result of beam_topk_rows over the logits
// (A[M,K] . W[V,K]^T) * rstd(A rows, when rms_eps > 0) + bias (when given), without the
// fp32 logits. topk <= 8. ws: lm_head_ws_bytes(M, V) bytes, 16-B aligned (per-tile partials
// and the per-row ban bitmap).
size_t lm_head_ws_bytes(int M, int V);
int lm_head_stages(int set);  // tile / ring / wave-grid config 0-5 (dev builds; release: 0); -1 reads
void lm_head_topk(const bf16* A, int lda, const bf16* W, int ldw, const float* bias, float rms_eps, int M, int V,
                  int K, int topk, const float* beam_scores, int eos, int mask_eos, const int32_t* bans, int nbmax,
                  const int32_t* seq, int seq_stride, int cur, int ngram, void* ws, float* out_score,
                  int32_t* out_token, hipStream_t stream);

// ------------------------------------------------------------- attention (K4)
// qkv: [B*S, 3*H*D] packed per token as [q(H*D) | k(H*D) | v(H*D)];
// lens: [B] valid key count per row (keys >= len masked); bias: optional
// additive fp32 [H, S, S] (T5 relative-position bias), may be null.
// out: [B*S, H*D]. D must be 64; S <= 512.
void attention_fwd(const bf16* qkv, const int32_t* lens, const float* bias, bf16* out, int B, int S, int H,
                   int D, float scale, hipStream_t stream);

// ------------------------------------------------------- normalisation (K2/K6b)
// out = LN(x (+ res)) * gamma + beta, rows of width N; fp32 statistics.
void layernorm_bf16(const bf16* x, const bf16* res, const float* gamma, const float* beta, bf16* out, int rows,
                    int N, float eps, hipStream_t stream);
// out = x * rsqrt(mean(x^2) + eps) * gamma (T5 RMSNorm, no mean subtraction)
void rmsnorm_bf16(const bf16* x, const float* gamma, bf16* out, int rows, int N, float eps,
                  hipStream_t stream);
// Fused BERT embedding: out[t] = LN(word[ids[t]] + pos[t % S] + type[tt[t]]); ids clamped to
// [0, vocab), type ids to [0, type_vocab).
void embed_layernorm(const int32_t* ids, const int32_t* type_ids, const bf16* word, const bf16* pos,
                     const bf16* type, const float* gamma, const float* beta, bf16* out, int B, int S, int N,
                     int vocab, int type_vocab, float eps, hipStream_t stream);
// LayerNorm folding: fin[m] = (rstd, rstd*mu) of rows of width K from the StatsOut
// partials part[slots][M][2] (sum, sumsq), slots summed in order (deterministic)
void ln_stats_finalize(const float* part, int slots, int M, int K, float eps, float* fin, hipStream_t stream);
// Plain embedding gather (T5 encoder/decoder input): out[t] = table[ids[t]] * scale
// LN(table[ids[r]] + pos[*step + pos_off]) per row (decoder input of a learned-position model at a
// device-side step; the layernorm_bf16 math, bit for bit)
void embed_pos_layernorm(const int32_t* ids, const bf16* table, const bf16* pos, const int32_t* step, int pos_off,
                         int npos, const float* gamma, const float* beta, bf16* out, int rows, int N, int vocab,
                         float eps, hipStream_t stream);
void embed_gather(const int32_t* ids, const bf16* table, bf16* out, int tokens, int N, int vocab,
                  hipStream_t stream);

// ----------------------------------------------------------- tokenizer (K1)
// Deterministic hash word-piece tokenizer (see agent_tpu_amd/tokenizer.py for
// the exact spec and the CPU twin). text: packed UTF-8 bytes; offsets[B+1].
void tokenize_hash(const uint8_t* text, const int32_t* offsets, int32_t* ids, int32_t* lens, int B, int S,
                   int vocab, int max_row_bytes, hipStream_t stream,
                   long long text_bytes);
// WordPiece vocabulary tokenizer ("atpu-wordpiece v1"): greedy longest match against the packed
// table of atpu/wordpiece.h. ``table``: the table on the launch device (16-byte aligned, resident
// while the kernel runs); ``header``: the host copy of its first 16 words, ``table_bytes`` its
// size. Output as tokenize_hash, with the special ids of the vocabulary.
void tokenize_wordpiece(const uint8_t* text, const int32_t* offsets, int32_t* ids, int32_t* lens, int B, int S,
                        const uint8_t* table, const int32_t* header, size_t table_bytes, int max_row_bytes,
                        hipStream_t stream, long long text_bytes);

// ------------------------------------------------------ re-ranker (rerank.hip)
// Pair rows "atpu-pair v1" (agent_tpu_amd/tokenizer.py pair_rows is the twin) from single-segment
// rows as the tokenizers emit them: passage row r with query row q = clamp(qidx[r], 0, Q-1) becomes
// [CLS] q_tok[0:nq] [SEP] p_tok[0:np] [SEP] [PAD]..., nq = min(lens_q[q]-2, mq, S-3),
// np = min(lens_p[r]-2, S-3-nq) (lens clamped into [2, S]); type_ids 1 on the passage segment and
// its [SEP]; lens = nq + np + 3. S >= 4, Q >= 1, mq >= 0; nothing outside the given rows is touched.
void pair_assemble(const int32_t* ids_q, const int32_t* lens_q, const int32_t* ids_p, const int32_t* lens_p,
                   const int32_t* qidx, int32_t* ids, int32_t* type_ids, int32_t* lens, int P, int Q, int S, int mq,
                   int cls, int sep, int pad, hipStream_t stream);
// Per-group top-k of scores [P]: group q is rows goff[q]..goff[q+1]-1 (goff [Q+1], clamped into
// [0, P]); idx [Q, k] is the index within the group, val [Q, k] the score, ordered by (value desc,
// index asc), +0.0 and -0.0 tie, a NaN ranks and is returned as -inf; a short group is padded
// with (-inf, -1). k in [1, 32].
void group_topk(const float* scores, const int32_t* goff, int32_t* idx, float* val, int P, int Q, int k,
                hipStream_t stream);

// ------------------------------------------------ late interaction (maxsim.hip)
// out [M, P] fp32 = the rows of x [M, P] (bf16 when is_bf16, else fp32) divided by max(||row||_2, 1e-12)
// (pool_embed's normalisation); the squares are summed in an order that depends on P alone.
// P % 64 == 0 in [64, 1024]; M == 0: no launch.
void token_unit(const void* x, float* out, int M, int P, int is_bf16, hipStream_t stream);
// scores [n]: pair p = (q = clamp(qidx[p], 0, Qn-1), d = clamp(didx[p], 0, Dn-1)) of the unit token
// vectors qv [Qn, S, P] / dv [Dn, S, P] (fp32, 16-byte aligned) gets
//   sum_{i < len_q} max_{j < len_d} <qv[q, i], dv[d, j]>      (lens clamped into [1, S])
// with every dot product in exact fp32 in sim_topk's k order, the max by select (tokens >= len never
// enter, whatever they hold) and the sum in fp32 in increasing i: a function of the pair's own rows
// alone. P % 64 == 0 in [64, 1024]; n == 0: no launch. A NaN in a live dot product: undefined.
void maxsim(const float* qv, const int32_t* lens_q, const float* dv, const int32_t* lens_d, const int32_t* qidx,
            const int32_t* didx, float* scores, int n, int Qn, int Dn, int S, int P, hipStream_t stream);

// ---------------------------------- late interaction over a resident index (maxsim_index.hip)
// The same score against a packed index: tok [T, P] (fp16 when is_f16, else fp32) holds the live unit token
// vectors of N passages back to back, passage p being rows off[p] .. off[p + 1] - 1 (off [N + 1] int64). Work
// item m is passage pidx[m] (m itself when pidx is null, M == N). All form (qoff and qsel null): out [Qn, M],
// every query against every item. List form: out [E], entry e in [qoff[m], qoff[m + 1]) is query qsel[e]
// against item m; an empty range is valid. One workgroup per item keeps the passage in LDS and loops over
// its queries. Exact fp32 dot products in a k order that depends on P and the dtype alone (fp32: maxsim's,
// the same bits); pidx, qsel, qoff, lens_q and the offsets are clamped before they form an address.
// P % 64 == 0 in [64, 1024]; M == 0: no launch.
void maxsim_index(const float* qv, const int32_t* lens_q, const void* tok, const int64_t* off, const int32_t* pidx,
                  const int32_t* qoff, const int32_t* qsel, float* out, int Qn, int S, int P, int64_t T, int N, int M, int E,
                  int is_f16, hipStream_t stream);

// ------------------------------------------- zero-shot classification (zeroshot.hip)
// Premise-first pair rows "atpu-premise v1" (agent_tpu_amd/tokenizer.py premise_rows is the twin): row r
// with text row t = clamp(tidx[r], 0, T-1) and hypothesis row h = clamp(hidx[r], 0, Hn-1) becomes
// [CLS] t_tok[0:nt] [SEP] h_tok[0:nh] [SEP] [PAD]..., nh = min(lens_h[h]-2, mh, S-3),
// nt = min(lens_t[t]-2, S-3-nh) (lens clamped into [2, S]); type_ids 1 on the hypothesis and its
// [SEP]; lens = nt + nh + 3. S >= 4, T >= 1, Hn >= 1, mh >= 0; nothing outside the P rows is touched.
void premise_assemble(const int32_t* ids_t, const int32_t* lens_t, const int32_t* ids_h, const int32_t* lens_h,
                      const int32_t* tidx, const int32_t* hidx, int32_t* ids, int32_t* type_ids, int32_t* lens, int P,
                      int T, int Hn, int S, int mh, int cls, int sep, int pad, hipStream_t stream);
// Label scores and the full ranking of every text's NLI logits pair [P, 2] = (entailment, contradiction):
// group t is rows goff[t]..goff[t+1]-1 (goff [T+1], clamped into [0, P]). mode 1, and any group of one:
// key e - c, score 1 / (1 + exp(-key)); mode 0: key e, score softmax over the group. A NaN logit (or
// difference) makes the key -inf and the score 0; a group whose best key is -inf scores 0 throughout.
// order [P] / score [P]: position goff[t] + r holds the group-local index and the score of the r-th
// element in (key desc, index asc) order, +0.0 and -0.0 tie. Positions outside every group are not written.
void nli_rank(const float* pair, const int32_t* goff, int32_t* order, float* score, int P, int T, int mode,
              hipStream_t stream);

// ------------------------------------------- question answering (span_head.hip)
// Start / end logits of the pair rows x [B*S, H] and the n best answer spans of each row's passage.
// With fin [B*S, 2] = (rstd, rstd*mu) the rows are raw and the LayerNorm is folded into the head:
// logit_c[j] = rstd_j (x_j . u_c) - (rstd_j mu_j) su_c + c_c; without it logit_c[j] = x_j . u_c + c_c.
// u [2, H], su [2], c [2] fp32. len = clamp(lens[b], 2, S); positions >= len have logit -inf.
// Candidates (i, j): lo <= i <= j <= hi, j - i < max_len, lo = the first position of type 1, hi =
// len - 2; value logit_0[i] + logit_1[j] (a NaN ranks as -inf), order (value desc, i * S + j asc).
// span [B, n, 2] passage-relative (i - lo, j - lo), score [B, n]; exhausted slots (-1, -1), -inf.
// null [B] = logit_0[0] + logit_1[0]; logits [B, S, 2] optional (null: not written).
// 4 <= S <= 512, H % 64 == 0 in [64, 1024], n in [1, 32], max_len in [1, S]; B == 0: no launch.
// own [B, 2] int32 (optional, null: none): row b proposes only starts i with lo + clamp(own0, 0, S)
// <= i < lo + clamp(own1, 0, S) (the window rows of window.hip); without it the launch is unchanged.
void span_topk(const bf16* x, const float* fin, const float* u, const float* su, const float* c,
               const int32_t* type_ids, const int32_t* lens, int32_t* span, float* score, float* null, float* logits,
               int B, int S, int H, int max_len, int n, hipStream_t stream, const int32_t* own = nullptr);

// ------------------------------------------- windows over long passages (window.hip)
// Window rows "atpu-window v1" (agent_tpu_amd/tokenizer.py window_rows is the twin). Window row r of
// pair p = clamp(win_pair[r], 0, Pp-1), question q = clamp(qidx[p], 0, Q-1), starting at passage
// token a = clamp(win_start[r], 0, max(T-1, 0)): [CLS] q_tok[0:nq] [SEP] p_tok[a : a+nw] [SEP] [PAD]...
// with nq = min(lens_q[q]-2, mq, S-3), cap = S-3-nq, T = lens_p[p]-2 (lens clamped into [2, S] /
// [2, L]; ids_q [Q, S], ids_p [Pp, L]), nw = min(cap, T-a); type_ids and lens as pair_assemble.
// own [R, 2] = the window-relative starts the row owns: step = min(stride, cap), h = (cap-step)/2,
// own0 = a == 0 ? 0 : h, own1 = a + cap >= T ? nw : step + h. Nothing outside the R rows is touched.
void window_assemble(const int32_t* ids_q, const int32_t* lens_q, const int32_t* ids_p, const int32_t* lens_p,
                     const int32_t* qidx, const int32_t* win_pair, const int32_t* win_start, int32_t* ids,
                     int32_t* type_ids, int32_t* lens, int32_t* own, int R, int Pp, int Q, int S, int L, int mq,
                     int stride, int cls, int sep, int pad, hipStream_t stream);
// The n best of every pair's window rows wrow[p] .. wrow[p+1]-1 (wrow [P+1], clamped into [0, R]) of
// span_w [R, n, 2] / score_w [R, n], ordered by (value desc, (row, slot) asc), a NaN ranks and is
// returned as -inf: span [P, n, 2] = the pick's span + start_w[row] (an exhausted slot stays (-1, -1)),
// score [P, n]; past the last element (-1, -1), -inf. null [P] = fminf over the rows' null_w in row
// order (+inf for no rows). n in [1, 32], R >= 1, R * n < 2^31.
void window_best(const int32_t* span_w, const float* score_w, const float* null_w, const int32_t* start_w,
                 const int32_t* wrow, int32_t* span, float* score, float* null, int R, int P, int n,
                 hipStream_t stream);

// ------------------------------------------- token classification (tag_head.hip)
// A label per text token j in [1, len - 2] of the rows x [B*S, H] ([CLS] text [SEP]) and the row's
// grouped entities. Logits as span_topk: with fin [B*S, 2] the rows are raw and logit_c[j] =
// rstd_j (x_j . u_c) - (rstd_j mu_j) su_c + c_c, without it x_j . u_c + c_c. u [L, H], su [L], c [L]
// fp32. y_j = argmax (logit desc, label asc, a NaN ranks as -inf, all NaN: 0), p_j = 1 / sum_c
// exp(logit_c - max) (a NaN adds 0; all NaN: p = 0). label_type [L] (-1: outside) and label_begin
// [L] drive the grouping: mode 0 one record per tagged token (first, first, label, 1); mode 1 a
// group starts when type >= 0 and (j == 1 or the type changes or begin) and runs to the next
// start or type change; mode 2 the same on word heads: a token with cont[ids[b, j]] != 0 (ids
// outside [0, V) and token 1: never) takes its head's label, never starts, always extends, and
// is not scored. ent [B, E, 4] = (first, last, type, n) text-relative, ent_sum [B, E] the fp32 sum
// of the n probabilities in token order; the first E groups in token order, count [B] the true
// number, unused slots (-1, -1, -1, 0) and 0.0. Optional (null: not written): label_out [B, S]
// (-1 outside the text), prob_out [B, S] (0 outside), logits_out [B, S, L] (-inf outside).
// ids / cont are read in mode 2 only. 3 <= S <= 512, H % 64 == 0 in [64, 1024], L in [1, 64],
// E in [1, 512]; B == 0: no launch.
void tag_entities(const bf16* x, const float* fin, const float* u, const float* su, const float* c,
                  const int32_t* lens, const int32_t* label_type, const int32_t* label_begin, const int32_t* ids,
                  const uint8_t* cont, int32_t* ent, float* ent_sum, int32_t* count, int32_t* label_out,
                  float* prob_out, float* logits_out, int B, int S, int H, int L, int V, int mode, int E,
                  hipStream_t stream);

// ------------------------------------------- masked-token prediction (fill.hip, mlm_head.hip)
// Mask rows "atpu-fill v1" (agent_tpu_amd/tokenizer.py fill_rows is the twin) from the single-segment
// rows ids_s [Ns, S] / lens_s [Ns] of the pieces between a text's mask tokens; the pieces of row b are
// segoff[b] .. segoff[b+1]-1 (segoff [B+1] clamped into [0, Ns], at most M + 1 of them are used):
// [CLS] seg_0 [MASK] seg_1 ... seg_m [SEP] [PAD]..., the concatenation cut to its first S - 2 tokens;
// lens = kept + 2; pos [B, M] = the row position of mask j, -1 where the row has fewer masks or the
// mask fell at or beyond position S - 1. S >= 3, M in [1, 16]; B == 0: no launch; nothing outside the
// given rows is touched.
void fill_assemble(const int32_t* ids_s, const int32_t* lens_s, const int32_t* segoff, int32_t* ids, int32_t* lens,
                   int32_t* pos, int B, int Ns, int S, int M, int cls, int sep, int pad, int mask, hipStream_t stream);
// xm [R, H] bf16 = the encoder row x[mrow[r] * S + pos[mrow[r], mord[r]]] of mask slot r (x [B*S, H],
// pos [B, M]). With fin [B*S, 2] = (rstd, rstd*mu) the rows are raw and the last LayerNorm is applied
// here: (x * rstd - rstd mu) * gamma + beta in fp32, rounded once; without it the rows are copied.
// A slot with mrow outside [0, B), mord outside [0, M) or pos outside [0, S) reads a clamped row,
// writes zeros and valid[r] = 0 (else 1). H % 64 == 0 in [64, 1024]; R == 0: no launch.
void mask_gather(const bf16* x, const float* fin, const float* gamma, const float* beta, const int32_t* pos,
                 const int32_t* mrow, const int32_t* mord, bf16* xm, int32_t* valid, int R, int B, int S, int M, int H,
                 hipStream_t stream);
// logit[r, v] = t[r] . E[v] + bias[v] (t [R, H] fp32, E [V, H] bf16 widened exactly, one fp32
// accumulator per (r, v) on the f32 MFMA, the k order a function of H alone, the bias added once
// after the chain), its log-sum-exp over all V tokens and its top k in the order (logit desc, token
// asc; a NaN ranks and returns as -inf and adds 0 to the sum). vocab_topk_partial fills the
// workspace ws [R * P * (k + 1), 2] fp32 (the [R, P, k] list entries, then the [R, P] (max, sum) pairs) with
// P = vocab_topk_splits(V) (a function of V alone: all four outputs of a
// slot have the same bits whatever R and the slot's place; mlm_head.hip's header); logits_out [R, V]
// optional (null: not written). vocab_topk_merge reduces them to tok [R, k] (-1 past V), logit [R, k]
// (-inf), prob [R, k] = exp(logit - lse) (0) and lse [R]; with lse_in [R] prob uses it instead of the
// launch's own; a slot with valid[r] == 0 (valid optional) returns (-1, -inf, 0) and lse = 0.
// H % 64 == 0 in [64, 1024], V >= 1, k in [1, 32]; R == 0: no launch. Nothing outside E[0:V] and
// bias[0:V] is read.
int vocab_topk_splits(int V);
void vocab_topk_partial(const float* t, const bf16* E, const float* bias, float* ws, float* logits_out, int R, int V,
                        int H, int k, hipStream_t stream);
void vocab_topk_merge(const float* ws, const int32_t* valid, const float* lse_in, int32_t* tok, float* logit,
                      float* prob, float* lse, int R, int V, int k, hipStream_t stream);

// ------------------------------------------------ classify head + top-k (K7)
// logits[b, c] = pooled[b] · Wc[c] + bc[c]; probs = softmax(logits);
// writes top-k (descending prob, ties -> lower index) and the full logits.
void classify_head_topk(const bf16* pooled, int ldp, const bf16* Wc, const float* bc, float* logits,
                        int32_t* topk_idx, float* topk_score, int B, int N, int C, int k, hipStream_t stream);

// ---------------------------------------------------- streaming reduce (K12)
// partial[4*blocks] doubles {count, sum, min, max}; finalize on host or via
// reduce_stats_finalize into out[4].
int reduce_stats_blocks(int64_t n);
void reduce_stats_f64(const double* x, int64_t n, double* partial, int blocks, hipStream_t stream);
void reduce_stats_f32(const float* x, int64_t n, double* partial, int blocks, hipStream_t stream);
void reduce_stats_finalize(const double* partial, int blocks, double* out, hipStream_t stream);
// acc[4] (+)= the reduction of a launch's block partials (first: overwrite); streamed reduces
void reduce_stats_accumulate(const double* partial, int blocks, double* acc, bool first, hipStream_t stream);
// K13+K12 over raw CSV records (runtime/risk_stream.cpp): record r is text[offs[r], offs[r+1]);
// field `col` parsed on the device (exact fast path), block partials [blocks][4] like
// reduce_stats_*; records the fast path cannot take are appended (global row row0 + r) to
// fb_rows (first fb_cap of them; *fb_count counts all) for the host to parse.
constexpr int kCsvMaxBlocks = 2048;
int csv_parse_blocks(int64_t n);
void csv_parse_reduce(const uint8_t* text, const uint32_t* offs, int n, int col, int64_t row0, double* partial,
                      int blocks, int* fb_count, int64_t* fb_rows, int fb_cap, hipStream_t stream);

}  // namespace atpu

namespace atpu {
// General strided form (T5 cross/causal attention): q rows b*Sq+t, k/v rows
// b*Skv+t; head h at column h*D of each row. ``bias`` is a dense fp32 [H, Sq, Skv]
// additive bias; ``bias_dist`` (exclusive with it) a bias by key-query distance,
// fp32 [H, Sq+Skv-1] with entry k - q + Sq - 1 (T5's relative position bias).
void attention_fwd_strided(const bf16* q, int ldq, const bf16* k, int ldk, const bf16* v, int ldv, bf16* out,
                           int ldo, const int32_t* lens, const float* bias, int B, int Sq, int Skv, int H, int D,
                           float scale, int causal, hipStream_t stream, const float* bias_dist = nullptr);
// 1 = long-sequence encoder attention on the double-buffered flash kernel (default), 0 = per-chunk kernel
int attention_flash_mode(int set);
}  // namespace atpu
