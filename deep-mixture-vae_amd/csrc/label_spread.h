// Label spreading on a symmetric sparse graph (label_spread.hip): the normalisation S = D^-1/2 W D^-1/2 of a CSR matrix and the
// iteration F <- alpha S F + (1 - alpha) Y.  Host-side launchers and the workspace layout.
#pragma once
#include "common.h"

namespace dmvae {

constexpr int SPREAD_MAX_N = 1 << 20;        // the cap of dmvae_knn, whose lists build the graph
constexpr int SPREAD_MIN_C = 2, SPREAD_MAX_C = 1024;
constexpr int SPREAD_ERR_INDEX = 1;          // a column index outside [0, N)
constexpr int SPREAD_ERR_LABEL = 2;          // a label outside {-1} u [0, C)
constexpr int SPREAD_WAVES = 4;              // waves per workgroup; they never wait for each other

// how a launch of the iteration is cut for C classes: a row's C columns are padded to Cp = 4 * nch floats, nch 16-byte chunks;
// G lanes (a power of two) share a row, one chunk each per pass, npass passes where nch > 64
struct SpreadShape { int Cp, nch, G, rows_per_wave, npass; };
SpreadShape spread_shape(int C);
int64_t spread_n_waves(int64_t N, int C);    // waves of one launch = per-wave maxima it leaves (a multiple of SPREAD_WAVES)

// 0, or DMVAE_EINVAL with the error text set (nothing is enqueued)
int graph_sym_normalize_launch(hipStream_t st, const int64_t* indptr, const int32_t* indices, const float* w, int N, int64_t nnz, float* s, float* r,
                               int32_t* err_flag);
int64_t label_spread_ws_bytes(int64_t N, int C);
int label_spread_launch(hipStream_t st, const int64_t* indptr, const int32_t* indices, const float* s, int N, int64_t nnz, const int32_t* labels, int C,
                        float alpha, int n_iter, const float* F_in, int64_t ld_in, float* F, int64_t ldf, float* change, void* ws, int64_t ws_bytes,
                        int32_t* err_flag);

}  // namespace dmvae
