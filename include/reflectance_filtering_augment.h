/* reflectance_filtering_augment.h -- C ABI of librf_augment_hip.so (gfx950 / MI355X): the transitive
 * hull of the judgement graphs of n photos, the reference's augment(comparisons, 'actual', 'min') of
 * training/createNumpyArrayWithComparisonsForIIW.py (supplementary section 1.1), in one call.
 *
 * The library is separate from librf_hip.so and librf_train_hip.so and shares no object with either.
 * It keeps NO state between calls - no tables, no side streams, no allocation - so there is nothing
 * to shut down.  The entry takes DEVICE pointers only, stages nothing, synchronises nothing, and
 * enqueues all its work on `stream` (a hipStream_t, NULL = the default stream), ordered like any
 * kernel launch; it is safe to capture into a graph.  Return codes are numerically those of
 * reflectance_filtering.h (RF_OK 0, RF_E_BADARG -1, RF_E_UNSUPPORTED -2, RF_E_HIP -4); every refusal
 * is decided on the host before any device work and leaves its text in rf_augment_last_error()
 * (thread-local).
 */
#ifndef REFLECTANCE_FILTERING_AUGMENT_H
#define REFLECTANCE_FILTERING_AUGMENT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_AUGMENT_VERSION 100
/* most nodes of one image: row k and column k of an iteration are staged in the 64 KB of LDS one
 * workgroup may have (12 bytes per present entry, two lists).  IIW's largest photo has 1,181
 * comparisons, so at most 2,362 nodes. */
#define RF_AUGMENT_MAX_NODES 2560

int rf_augment_version(void);
const char *rf_augment_last_error(void);

/* The hull of n judgement graphs.  Image b has N_b = node_offsets[b+1] - node_offsets[b] nodes,
 * numbered 0..N_b-1, and the edges [edge_offsets[b], edge_offsets[b+1]).
 *
 *   edges          [E][3]  int32    (from node, to node, relation): relation 0 = about equal,
 *                                   2 = `to` is darker, the reference's unified form
 *   edge_weights   [E]     float64
 *   edge_offsets   [n+1]   int32    absolute offsets into edges / edge_weights
 *   node_offsets   [n+1]   int32    running sum of N_b
 *   matrix_offsets [n+1]   int64    running sum of N_b * N_b
 *   out_offsets    [n+1]   int64    running sum of N_b * (N_b - 1) / 2
 *   node_point     [total_nodes] int32 or NULL: written in place of node i of image b is
 *                                   node_point[node_offsets[b] + i]; NULL writes the node id
 *   coins          [total_matrix] uint8 or NULL (= all zero): see S3
 *   n, max_nodes (the largest N_b), total_nodes, total_edges, total_matrix, cap: host copies of
 *                                   node_offsets[n], edge_offsets[n], matrix_offsets[n] and the
 *                                   rows of comps_out / weights_out, cap >= out_offsets[n]
 *   comps_out      [cap][3] int32   (index 1, index 2, darker) - darker is the relation, 0 or 2 -
 *   weights_out    [cap]    float64 and counts_out [n] int32: image b's list is the counts_out[b]
 *                                   rows from row out_offsets[b]; the rows behind it up to
 *                                   out_offsets[b+1] are not written.  This is the comparison format
 *                                   of rf_train_whdr_hinge_points_f32.
 *
 * The caller promises that the ordered pairs (from, to) of an image's edges are distinct, that none
 * has from == to, that every node id lies in [0, N_b) and that max_nodes and the totals are what the
 * device arrays say.  Anything else is the caller's error.
 *
 * S1 matrix.  Relation and weight start absent everywhere; each edge sets (from, to).
 * S2 closure.  For k = 0..N-1 in order, for all i != j: c = min(w[i][k], w[k][j]) if both are
 *    present; if c is present and w[i][j] is absent or w[i][j] < c (strictly), w[i][j] = c and
 *    rel[i][j] = rel[i][k] if rel[i][k] == rel[k][j], else 2.  Row k and column k are read as they
 *    stood at the start of iteration k (the diagonal stays absent, so iteration k never writes them).
 * S3 resolution.  Once per unordered pair i < j with both directions present: relations (2,2), (2,0)
 *    or (0,2): (j,i) is dropped if w[i][j] > w[j][i], else (i,j) (a tie drops (i,j)); relations
 *    (0,0): (j,i) is dropped if the byte coins[matrix_offsets[b] + i * N + j] is non-zero, else
 *    (i,j).  A non-zero coin stands for the reference's np.random.rand() > 0.5.
 * S4 output.  The remaining entries in row-major (i, j) order as (point of i, point of j, relation)
 *    and weight; counts_out[b] is their number, at most N (N - 1) / 2.
 * S5 Weights are float64 from end to end; min and the comparisons are exact.  No atomics.  The
 *    result is the same bits from run to run and does not depend on what the workspace held.
 *
 * One workgroup of 1,024 per image walks k over matrices kept in the workspace (8 + 1 bytes per
 * entry); a photo of many nodes takes as long as it takes while the small ones have finished.
 *
 * workspace: rf_augment_hull_workspace_bytes(total_matrix) bytes, 16-byte aligned; a NULL, smaller
 * or misaligned one is RF_E_BADARG.  n == 0 is RF_OK whatever the pointers; NULL pointers (other
 * than node_point and coins), negative sizes, totals larger than n images of max_nodes can have and
 * cap < (total_matrix - total_nodes) / 2 are RF_E_BADARG; max_nodes > RF_AUGMENT_MAX_NODES, n >= 2^22
 * total_nodes or total_edges >= 2^31 and total_matrix > 2^40 are RF_E_UNSUPPORTED.  An image without
 * edges (and so without nodes) yields count 0.  The workspace query returns 0 where the entry would
 * refuse total_matrix.
 */
size_t rf_augment_hull_workspace_bytes(long long total_matrix);
int rf_augment_hull_f64(const int *edges, const double *edge_weights, const int *edge_offsets,
                        const int *node_offsets, const long long *matrix_offsets,
                        const long long *out_offsets, const int *node_point,
                        const unsigned char *coins, int n, int max_nodes, long long total_nodes,
                        long long total_edges, long long total_matrix, long long cap, int *comps_out,
                        double *weights_out, int *counts_out, void *workspace,
                        size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
