// rf_augment_hull.hip -- the transitive hull of judgement graphs, one workgroup per image.
//
// Restates augment() / warshall() of the reference's training/createNumpyArrayWithComparisonsForIIW.py
// with consolidation 'min' (S1..S4 of the header).  Iteration k of the reference's triple loop leaves
// row k and column k alone: the diagonal is never set, so every candidate that would land in them
// has an absent operand.  All (i, j) of one k are therefore independent, and the workgroup does
// per k:
//   stage    the present entries of column k (rows i with w[i][k]) and of row k (columns j with
//            w[k][j]) into two compact LDS lists, in ascending order, by ballot and a prefix over
//            the per-wave counts (no atomics);
//   update   wave by wave one listed row i, lanes over the listed columns j.
// Global writes of one wave are read by the other waves of the workgroup an iteration later, behind
// a workgroup barrier: all waves of a workgroup share their CU's L1, and __syncthreads() carries
// the workgroup-scope release / acquire.  Nothing is handed to another workgroup.
// Afterwards the same workgroup resolves the two-way pairs (S3, a pure function of the matrix)
// and writes the survivors in row-major order: per-row counts, a prefix, an ordered write (S4).
#include "rf_augment_common.hpp"

namespace rfa {
namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxNodes = RF_AUGMENT_MAX_NODES;
constexpr int kRounds = (kMaxNodes + kThreads - 1) / kThreads;     // staging rounds of 1,024 entries
constexpr int kChunks = kRounds * kWaves;                         // 64-entry chunks of a list
constexpr unsigned char kAbsent = 0xFF;
constexpr long long kMaxMatrix = 1ll << 40;

static_assert(kMaxNodes < 65536, "a list entry packs the node id into 16 bits");

struct Args {
    const int *edges;
    const double *edge_weights;
    const int *edge_offsets;
    const int *node_offsets;
    const long long *matrix_offsets;
    const long long *out_offsets;
    const int *node_point;
    const unsigned char *coins;
    int *comps_out;
    double *weights_out;
    int *counts_out;
    double *w;               // workspace: weights [total_matrix]
    unsigned char *rel;      // workspace: relations [total_matrix], kAbsent = no entry
};

// Does entry (i, j), i != j, remain after S3?  r1 returns its relation.
__device__ __forceinline__ bool survives(const double *W, const unsigned char *R,
                                         const unsigned char *coins, int N, int i, int j,
                                         unsigned char &r1)
{
    r1 = R[(size_t)i * N + j];
    if (r1 == kAbsent)
        return false;
    const unsigned char r2 = R[(size_t)j * N + i];
    if (r2 == kAbsent)
        return true;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const size_t up = (size_t)lo * N + hi, down = (size_t)hi * N + lo;
    bool drop_down;          // (hi, lo) is the one dropped
    if (r1 == 0 && r2 == 0)
        drop_down = coins != nullptr && coins[up] != 0;
    else
        drop_down = W[up] > W[down];
    return (i < j) == drop_down;
}

__global__ __launch_bounds__(kThreads) void hull_kernel(Args a)
{
    __shared__ double s_w[2][kMaxNodes];      // list 0: column k (w[i][k]); list 1: row k (w[k][j])
    __shared__ int s_id[2][kMaxNodes];        // node id | relation << 16
    __shared__ int s_cnt[2][kChunks];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int n0 = a.node_offsets[b];
    const int N = a.node_offsets[b + 1] - n0;
    if (N <= 0 || N > kMaxNodes) {            // (more than the limit: the caller's error, no LDS for it)
        if (t == 0)
            a.counts_out[b] = 0;
        return;
    }
    const long long m0 = a.matrix_offsets[b];
    double *W = a.w + m0;
    unsigned char *R = a.rel + m0;
    const unsigned char *coins = a.coins ? a.coins + m0 : nullptr;
    const size_t NN = (size_t)N * N;

    // S1: everything absent (weights of absent entries are never read), then the edges
    {
        size_t head = (size_t)(-(uintptr_t)R & 15);
        if (head > NN)
            head = NN;
        const size_t quads = (NN - head) / 16;
        for (size_t e = t; e < head; e += kThreads)
            R[e] = kAbsent;
        uint4 *R16 = reinterpret_cast<uint4 *>(R + head);
        const uint4 all = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
        for (size_t e = t; e < quads; e += kThreads)
            R16[e] = all;
        for (size_t e = head + quads * 16 + t; e < NN; e += kThreads)
            R[e] = kAbsent;
    }
    __syncthreads();
    for (int e = a.edge_offsets[b] + t; e < a.edge_offsets[b + 1]; e += kThreads) {
        const int from = a.edges[(size_t)e * 3], to = a.edges[(size_t)e * 3 + 1];
        if (from < 0 || from >= N || to < 0 || to >= N || from == to)
            continue;                          // the caller's error: nothing written outside the matrix
        W[(size_t)from * N + to] = a.edge_weights[e];
        R[(size_t)from * N + to] = a.edges[(size_t)e * 3 + 2] == 0 ? 0 : 2;
    }
    __syncthreads();

    // S2
    for (int k = 0; k < N; k++) {
        int rel_a[kRounds], rel_b[kRounds], pos_a[kRounds], pos_b[kRounds];
#pragma unroll
        for (int r = 0; r < kRounds; r++) {
            rel_a[r] = rel_b[r] = -1;
            if (r * kThreads < N) {
                const int e = r * kThreads + t;
                if (e < N) {
                    const unsigned char x = R[(size_t)e * N + k], y = R[(size_t)k * N + e];
                    if (x != kAbsent)
                        rel_a[r] = x;
                    if (y != kAbsent)
                        rel_b[r] = y;
                }
                const unsigned long long ma = __ballot(rel_a[r] >= 0), mb = __ballot(rel_b[r] >= 0);
                pos_a[r] = __popcll(ma & below);
                pos_b[r] = __popcll(mb & below);
                if (lane == 0) {
                    s_cnt[0][r * kWaves + wave] = __popcll(ma);
                    s_cnt[1][r * kWaves + wave] = __popcll(mb);
                }
            }
        }
        __syncthreads();
        int na = 0, nb = 0;
#pragma unroll
        for (int r = 0; r < kRounds; r++) {
            if (r * kThreads < N) {
                const int e = r * kThreads + t, c = r * kWaves + wave;
                int off_a = na, off_b = nb;
                for (int q = 0; q < kWaves; q++) {
                    const int ca = s_cnt[0][r * kWaves + q], cb = s_cnt[1][r * kWaves + q];
                    na += ca;
                    nb += cb;
                    if (r * kWaves + q < c) {
                        off_a += ca;
                        off_b += cb;
                    }
                }
                if (rel_a[r] >= 0) {
                    s_id[0][off_a + pos_a[r]] = e | (rel_a[r] << 16);
                    s_w[0][off_a + pos_a[r]] = W[(size_t)e * N + k];
                }
                if (rel_b[r] >= 0) {
                    s_id[1][off_b + pos_b[r]] = e | (rel_b[r] << 16);
                    s_w[1][off_b + pos_b[r]] = W[(size_t)k * N + e];
                }
            }
        }
        __syncthreads();
        if (nb > 0) {
            for (int ri = wave; ri < na; ri += kWaves) {
                const int ia = s_id[0][ri], i = ia & 0xFFFF, rel_ik = ia >> 16;
                const double wik = s_w[0][ri];
                double *Wi = W + (size_t)i * N;
                unsigned char *Ri = R + (size_t)i * N;
                for (int cj = lane; cj < nb; cj += 64) {
                    const int jb = s_id[1][cj], j = jb & 0xFFFF, rel_kj = jb >> 16;
                    if (j == i)
                        continue;
                    const double wkj = s_w[1][cj];
                    const double c = wkj < wik ? wkj : wik;
                    if (Ri[j] == kAbsent || Wi[j] < c) {
                        Wi[j] = c;
                        Ri[j] = (unsigned char)(rel_ik == rel_kj ? rel_ik : 2);
                    }
                }
            }
        }
        __syncthreads();
    }

    // S3 + S4: survivors per row, their prefix, the ordered write
    int *row_count = s_id[0], *row_start = s_id[1];
    for (int i = wave; i < N; i += kWaves) {
        int count = 0;
        for (int j0 = 0; j0 < N; j0 += 64) {
            const int j = j0 + lane;
            unsigned char r1;
            const bool keep = j < N && j != i && survives(W, R, coins, N, i, j, r1);
            count += __popcll(__ballot(keep));
        }
        if (lane == 0)
            row_count[i] = count;
    }
    __syncthreads();
    if (t == 0) {
        int sum = 0;
        for (int i = 0; i < N; i++) {
            row_start[i] = sum;
            sum += row_count[i];
        }
        a.counts_out[b] = sum;
    }
    __syncthreads();
    const long long o0 = a.out_offsets[b];
    for (int i = wave; i < N; i += kWaves) {
        long long row = o0 + row_start[i];
        const int pi = a.node_point ? a.node_point[n0 + i] : i;
        for (int j0 = 0; j0 < N; j0 += 64) {
            const int j = j0 + lane;
            unsigned char r1 = 0;
            const bool keep = j < N && j != i && survives(W, R, coins, N, i, j, r1);
            const unsigned long long m = __ballot(keep);
            if (keep) {
                const long long at = row + __popcll(m & below);
                a.comps_out[at * 3] = pi;
                a.comps_out[at * 3 + 1] = a.node_point ? a.node_point[n0 + j] : j;
                a.comps_out[at * 3 + 2] = r1;
                a.weights_out[at] = W[(size_t)i * N + j];
            }
            row += __popcll(m);
        }
    }
}

size_t matrix_bytes(long long total_matrix)
{
    return ((size_t)total_matrix * 8 + 15) & ~(size_t)15;
}

}  // namespace
}  // namespace rfa

extern "C" size_t rf_augment_hull_workspace_bytes(long long total_matrix)
{
    using namespace rfa;
    if (total_matrix < 0 || total_matrix > kMaxMatrix)
        return 0;
    return matrix_bytes(total_matrix) + (((size_t)total_matrix + 15) & ~(size_t)15) + 16;
}

extern "C" int rf_augment_hull_f64(const int *edges, const double *edge_weights,
                                   const int *edge_offsets, const int *node_offsets,
                                   const long long *matrix_offsets, const long long *out_offsets,
                                   const int *node_point, const unsigned char *coins, int n,
                                   int max_nodes, long long total_nodes, long long total_edges,
                                   long long total_matrix, long long cap, int *comps_out,
                                   double *weights_out, int *counts_out, void *workspace,
                                   size_t workspace_bytes, void *stream_)
{
    using namespace rfa;
    const char *who = "rf_augment_hull_f64";
    if (n == 0)  // an empty list is valid whatever the (possibly NULL) pointers are
        return kOk;
    if (n < 0 || max_nodes < 0 || total_nodes < 0 || total_edges < 0 || total_matrix < 0 || cap < 0)
        return fail(kBadArg, "%s: bad size n=%d max_nodes=%d total_nodes=%lld total_edges=%lld "
                    "total_matrix=%lld cap=%lld", who, n, max_nodes, total_nodes, total_edges,
                    total_matrix, cap);
    if (!edges || !edge_weights || !edge_offsets || !node_offsets || !matrix_offsets ||
        !out_offsets || !comps_out || !weights_out || !counts_out)
        return fail(kBadArg, "%s: NULL pointer", who);
    if (max_nodes > kMaxNodes)
        return fail(kUnsupported, "%s: an image of %d nodes, the limit is %d", who, max_nodes,
                    kMaxNodes);
    // a workgroup per image: gridDim x blockDim stays below 2^32 work-items
    if ((unsigned long long)n * kThreads >= (1ull << 32))
        return fail(kUnsupported, "%s: too many images for one launch", who);
    if (total_nodes >= (1ll << 31) || total_edges >= (1ll << 31) || total_matrix > kMaxMatrix)
        return fail(kUnsupported, "%s: node and edge offsets are 32-bit, matrices hold 2^40 entries",
                    who);
    if (total_nodes > (long long)n * max_nodes ||
        total_matrix > (long long)n * max_nodes * max_nodes || total_matrix < total_nodes)
        return fail(kBadArg, "%s: totals larger than %d images of at most %d nodes have", who, n,
                    max_nodes);
    if (cap < (total_matrix - total_nodes) / 2)
        return fail(kBadArg, "%s: cap=%lld is below the %lld rows the images may need", who, cap,
                    (total_matrix - total_nodes) / 2);
    const size_t need = rf_augment_hull_workspace_bytes(total_matrix);
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < need)
        return fail(kBadArg, "%s: the workspace must be 16-byte aligned and hold %zu bytes", who,
                    need);
    Args a;
    a.edges = edges;
    a.edge_weights = edge_weights;
    a.edge_offsets = edge_offsets;
    a.node_offsets = node_offsets;
    a.matrix_offsets = matrix_offsets;
    a.out_offsets = out_offsets;
    a.node_point = node_point;
    a.coins = coins;
    a.comps_out = comps_out;
    a.weights_out = weights_out;
    a.counts_out = counts_out;
    a.w = static_cast<double *>(workspace);
    a.rel = static_cast<unsigned char *>(workspace) + matrix_bytes(total_matrix);
    hipLaunchKernelGGL(hull_kernel, dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream_, a);
    RFA_HIP_CHECK(hipGetLastError());
    return kOk;
}
