/* escgnn_lappe.h - the Laplacian positional encoding's entry points of libescgnn_hip.so (csrc/lappe.hip): the batched
 * eigen-decomposition of graph Laplacians, the row gather from a resident PE table and the DeepSet LapPE encoder with its
 * backward; a fifth extension header next to escgnn_hip.h, escgnn_subgraphs.h, escgnn_i2gnn.h, escgnn_gineplus.h and
 * escgnn_gps.h.  Same conventions and the same grammar: esc-gnn_amd/_abi.py reads THIS FILE too and derives the binding of
 * these functions from it (esc-gnn_amd/_native.py, LAPPE_SIGNATURES).  Functions only, no struct, no constant:
 * ESC_ABI_VERSION is not concerned. */
#ifndef ESCGNN_LAPPE_H
#define ESCGNN_LAPPE_H
#include "escgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched Laplacian eigen-decomposition (reference GraphGPS/graphgps/transform/posenc_stats.py:40-73,149-182,353-401
 * with laplacian_norm none and eigvec_norm L2).  One workgroup per graph of a ragged set: a collated batch, or a
 * store's whole split in one launch.
 * src, dst  int64 [E]: the two rows of edge_index.  edges_local != 0: the ends are graph-local node ids (a store's flat
 *           arrays); 0: they are rows of the batch (a collated edge_index).
 * node_ptr  int64 [G+1]: the nodes of graph g are the rows [node_ptr[g], node_ptr[g+1]), n = their number.
 * edge_ptr  int64 [G+1]: its edges are [edge_ptr[g], edge_ptr[g+1]) - contiguous per graph.
 * A_ij = 1 if an edge (i, j) or (j, i) with i != j is present (plain stores of one value, no atomics: self-loops are dropped
 * and a repeated edge counts once - equal to the reference on simple graphs, directed or not; multigraphs, whose duplicates
 * the reference sums, are out of scope).  L = D - A in fp64, decomposed by the one-sided Jacobi of csrc/jacobi_pinv.h (for a
 * positive semi-definite matrix the right singular vectors are eigenvectors and the column norms of L V the eigenvalues).
 * Eigenvalues ascending (equal ones in column order), clamped at 0, the max_freqs = K smallest kept; every kept eigenvector
 * divided by max(||v||_2, 1e-12).
 *   eigvecs [N, K] fp32: eigvecs[i, j] = component of node i in the j-th eigenvector of its graph;
 *   eigvals [N, K] fp32: the graph's eigenvalues repeated on each of its rows;
 *   in both, columns j >= n of a graph with n < K nodes are NaN.
 * The signs, and the basis inside an eigenspace of equal eigenvalues, are whatever the deterministic algorithm yields.
 * max_nodes: the largest n, told by the caller (nothing is read back); it sizes the LDS.  The two n x n fp64 matrices of a
 * graph live in LDS (column stride n | 1 doubles) for n <= esc_laplacian_eig_lds_nodes() = 90: the largest n with
 * 2 * n * (n | 1) * 8 bytes inside the 128 KiB the workgroup asks for at most - a launch asks for what max_nodes needs, not
 * for the limit.  Larger graphs, up to esc_laplacian_eig_max_nodes() = 256, keep them in `scratch`: graph g owns the
 * 2 * n * (max_nodes | 1) doubles from 2 * node_ptr[g] * (max_nodes | 1) on; esc_laplacian_eig_scratch_bytes(N, max_nodes)
 * is what the launch needs (0 when max_nodes <= the LDS size; scratch may then be NULL).  Which of the two a graph takes
 * depends on its own size alone, and its result on nothing else in the launch: bit-equal alone and inside any batch.
 * Limits (the message names them; checked on the host before anything is launched): max_nodes <= 256, 1 <= K <= 32,
 * scratch_bytes at least the query's answer.
 * A graph that contradicts what the host was told - more nodes than max_nodes, a node or edge range that is negative or
 * leaves [0, N) / [0, E), an edge end outside the graph - is skipped by its workgroup: nothing is read or written out of
 * bounds, its rows stay unwritten.  Empty graphs, G == 0 and N == 0 are legal and write nothing.
 * Launches: 1.  No atomics, no cross-workgroup sums: bit-identical run to run. */
int64_t esc_laplacian_eig_max_nodes(void);
int64_t esc_laplacian_eig_lds_nodes(void);
int64_t esc_laplacian_eig_scratch_bytes(int64_t N, int64_t max_nodes);
int esc_laplacian_eig(const int64_t* src, const int64_t* dst, int64_t E, const int64_t* node_ptr, const int64_t* edge_ptr,
                      int64_t G, int64_t N, int edges_local, int max_freqs, int64_t max_nodes, void* scratch,
                      int64_t scratch_bytes, float* eigvecs, float* eigvals, void* stream);

/* ---- what the reference's collate does to the EigVecs / EigVals keys, off a resident table: one launch, one workgroup per
 * graph of the batch.  vecs_all, vals_all [N_all, K]: the table of a whole split; node_ptr_all int64 [G_all+1]: its node
 * ranges; graph_ids int64 [B] (device): the batch's graphs in batch order; graph_ptr int32 [B+1]: the batch's node ranges.
 * Rows [graph_ptr[b], graph_ptr[b+1]) of vecs / vals [N, K] receive rows [node_ptr_all[id], node_ptr_all[id+1]) of the table.
 * The ids live on the device: the caller checks them on the host (ops.lappe_gather does); a workgroup whose id is out of
 * range, or whose two ranges differ in length or leave their arrays, copies nothing. */
int esc_lappe_gather(const float* vecs_all, const float* vals_all, const int64_t* node_ptr_all, int64_t G_all, int64_t N_all,
                     const int64_t* graph_ids, const int32_t* graph_ptr, int64_t B, int64_t N, int K, float* vecs,
                     float* vals, void* stream);

/* ---- the DeepSet LapPE encoder (reference graphgps/encoder/laplace_pos_encoder.py:94-132 for model DeepSet, layers 2,
 * post_layers 0, raw_norm_type none).  For node i and frequency j:  v = eigvecs[i,j] * sign[j],  l = eigvals[i,j], NaNs in
 * (v, l) replaced by 0;  h = ReLU(W1 ReLU(WA [v, l] + bA) + b1) with WA [2P, 2], bA [2P], W1 [P, 2P], b1 [P] (row-major,
 * torch's Linear layout);  out[i, :] = sum over the j whose eigvecs[i,j] is not NaN of h.
 * signs [K] fp32 or NULL for none.  out [N, P] rows with leading dimension ld_out (a column slice of a wider buffer).
 * One launch, one thread per node, the weights staged in LDS.
 * Limits (the message names them): P a multiple of 4 and at most 32, 1 <= K <= 32, ld_out >= P. */
int esc_lappe_encode_fwd(const float* eigvecs, const float* eigvals, const float* signs, const float* wA, const float* bA,
                         const float* w1, const float* b1, int64_t N, int K, int P, float* out, int64_t ld_out, void* stream);
/* The parameter gradients of the same expression given d_out [N, P] (leading dimension ld_dout); the hidden activations are
 * recomputed, nothing is saved, and the eigen-data get no gradient.  Launch 1: workgroup w takes the rows
 * [w * R, (w + 1) * R), R = esc_lappe_encode_block_rows(), and writes its partial of all 2 P^2 + 7 P parameter gradients to
 * scratch [ceil(N / R), 2 P^2 + 7 P] in the order (d_wA, d_bA, d_w1, d_b1); launch 2 adds the partials in ascending w.
 * esc_lappe_encode_scratch_floats(N, P) floats of scratch are needed.  No atomics: bit-identical run to run; a term whose
 * eigvecs entry is NaN contributes exact zeros.  N == 0 writes zero gradients (one launch). */
int64_t esc_lappe_encode_block_rows(void);
int64_t esc_lappe_encode_scratch_floats(int64_t N, int P);
int esc_lappe_encode_bwd(const float* eigvecs, const float* eigvals, const float* signs, const float* wA, const float* bA,
                         const float* w1, const float* b1, const float* d_out, int64_t ld_dout, int64_t N, int K, int P,
                         float* scratch, int64_t scratch_floats, float* d_wA, float* d_bA, float* d_w1, float* d_b1,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
