// activation.hip — an activation with no BatchNorm in front of it: the bare ELU / ReLU of the CSL model's GINEConv MLPs
// (Linear, ELU, Linear, ELU) and of its head (elu(lin1)), reference run_csl.py:148-172,219.
//
// Same expressions as norm.hip's act_fwd / act_grad_from_out (codes 1 = ReLU, 2 = ELU(alpha = 1)); the backward works from
// the forward OUTPUT, so only Y is kept.  HBM-bound elementwise work: 16 B per lane where the layout allows it, at most
// 2 048 workgroups, grid-stride, 64-bit element indices.  Every element is read and written by the same thread, so Y may
// alias X and dX may alias dY (no __restrict__ on those).
#include "common.h"

namespace esc {

template <int ACT>
__device__ __forceinline__ float bare_act_fwd(float v) {
  if constexpr (ACT == 1) return fmaxf(v, 0.f);
  else return v > 0.f ? v : expm1f(v);
}
// dX = dY * d act / d v through the output: relu [y > 0]; elu y > 0 ? 1 : y + 1.  The factors 1 and 0 are applied as a
// select (a gradient behind a dead ReLU is +0 whatever dY holds).
template <int ACT>
__device__ __forceinline__ float bare_act_bwd(float y, float g) {
  if constexpr (ACT == 1) return y > 0.f ? g : 0.f;
  else return y > 0.f ? g : g * (y + 1.f);
}

// item i of `items` covers VEC consecutive columns; FLAT: every leading dimension equals C, the matrix is one run
template <int VEC, bool FLAT>
__device__ __forceinline__ void act_offsets(int64_t i, int64_t row_items, int64_t ld_a, int64_t ld_b, int64_t ld_c, int64_t& a,
                                            int64_t& b, int64_t& c) {
  if constexpr (FLAT) {
    a = b = c = i * VEC;
  } else {
    const int64_t r = i / row_items;
    const int64_t col = (i - r * row_items) * VEC;
    a = r * ld_a + col;
    b = r * ld_b + col;
    c = r * ld_c + col;
  }
}

template <int ACT, int VEC, bool FLAT>
__global__ __launch_bounds__(256) void act_fwd_kernel(const float* X, int64_t ldx, int64_t items, int64_t row_items, float* Y,
                                                      int64_t ldy) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += step) {
    int64_t ox, oy, unused;
    act_offsets<VEC, FLAT>(i, row_items, ldx, ldy, ldy, ox, oy, unused);
    if constexpr (VEC == 4) {
      const float4 v = *reinterpret_cast<const float4*>(X + ox);
      *reinterpret_cast<float4*>(Y + oy) =
          make_float4(bare_act_fwd<ACT>(v.x), bare_act_fwd<ACT>(v.y), bare_act_fwd<ACT>(v.z), bare_act_fwd<ACT>(v.w));
    } else {
      Y[oy] = bare_act_fwd<ACT>(X[ox]);
    }
  }
}

template <int ACT, int VEC, bool FLAT>
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* Y, int64_t ldy, const float* dY, int64_t ldg,
                                                      int64_t items, int64_t row_items, float* dX, int64_t ldd) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += step) {
    int64_t oy, og, od;
    act_offsets<VEC, FLAT>(i, row_items, ldy, ldg, ldd, oy, og, od);
    if constexpr (VEC == 4) {
      const float4 y = *reinterpret_cast<const float4*>(Y + oy);
      const float4 g = *reinterpret_cast<const float4*>(dY + og);
      *reinterpret_cast<float4*>(dX + od) =
          make_float4(bare_act_bwd<ACT>(y.x, g.x), bare_act_bwd<ACT>(y.y, g.y), bare_act_bwd<ACT>(y.z, g.z), bare_act_bwd<ACT>(y.w, g.w));
    } else {
      dX[od] = bare_act_bwd<ACT>(Y[oy], dY[og]);
    }
  }
}

constexpr int64_t ACT_MAX_BLOCKS = 2048;        // 256 CUs x 8 workgroups of 256 threads: the rest is grid-stride

inline unsigned act_grid(int64_t items) { return (unsigned)(cdiv(items, 256) < ACT_MAX_BLOCKS ? cdiv(items, 256) : ACT_MAX_BLOCKS); }

template <int ACT>
void launch_act_fwd(const float* X, int64_t ldx, int64_t M, int64_t C, float* Y, int64_t ldy, hipStream_t s) {
  const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned16(X) && aligned16(Y);
  const bool flat = (ldx == C && ldy == C) || M == 1;
  const int64_t row_items = vec ? C / 4 : C, items = M * row_items;
  const dim3 grid(act_grid(items)), block(256);
  if (vec && flat) esc::launch(ESC_K_NORM, act_fwd_kernel<ACT, 4, true>, grid, block, 0, s, X, ldx, items, row_items, Y, ldy);
  else if (vec) esc::launch(ESC_K_NORM, act_fwd_kernel<ACT, 4, false>, grid, block, 0, s, X, ldx, items, row_items, Y, ldy);
  else if (flat) esc::launch(ESC_K_NORM, act_fwd_kernel<ACT, 1, true>, grid, block, 0, s, X, ldx, items, row_items, Y, ldy);
  else esc::launch(ESC_K_NORM, act_fwd_kernel<ACT, 1, false>, grid, block, 0, s, X, ldx, items, row_items, Y, ldy);
}

template <int ACT>
void launch_act_bwd(const float* Y, int64_t ldy, const float* dY, int64_t ldg, int64_t M, int64_t C, float* dX, int64_t ldd,
                    hipStream_t s) {
  const bool vec = C % 4 == 0 && ldy % 4 == 0 && ldg % 4 == 0 && ldd % 4 == 0 && aligned16(Y) && aligned16(dY) && aligned16(dX);
  const bool flat = (ldy == C && ldg == C && ldd == C) || M == 1;
  const int64_t row_items = vec ? C / 4 : C, items = M * row_items;
  const dim3 grid(act_grid(items)), block(256);
  if (vec && flat) esc::launch(ESC_K_NORM, act_bwd_kernel<ACT, 4, true>, grid, block, 0, s, Y, ldy, dY, ldg, items, row_items, dX, ldd);
  else if (vec) esc::launch(ESC_K_NORM, act_bwd_kernel<ACT, 4, false>, grid, block, 0, s, Y, ldy, dY, ldg, items, row_items, dX, ldd);
  else if (flat) esc::launch(ESC_K_NORM, act_bwd_kernel<ACT, 1, true>, grid, block, 0, s, Y, ldy, dY, ldg, items, row_items, dX, ldd);
  else esc::launch(ESC_K_NORM, act_bwd_kernel<ACT, 1, false>, grid, block, 0, s, Y, ldy, dY, ldg, items, row_items, dX, ldd);
}

}  // namespace esc

using namespace esc;

extern "C" {

int esc_act_fwd(const float* X, int64_t ld_x, int64_t M, int64_t C, int act, float* Y, int64_t ld_y, void* stream) {
  ESC_REQUIRE(act == 1 || act == 2, "esc_act_fwd: activation code %d (1 = ReLU, 2 = ELU)", act);
  ESC_REQUIRE(M >= 0 && C >= 0, "esc_act_fwd: negative size M=%ld C=%ld", (long)M, (long)C);
  ESC_REQUIRE(ld_x >= C && ld_y >= C, "esc_act_fwd: leading dimensions %ld / %ld below C=%ld", (long)ld_x, (long)ld_y, (long)C);
  if (M == 0 || C == 0) return ESC_OK;
  ESC_REQUIRE(X && Y, "esc_act_fwd: null pointer");
  ESC_REQUIRE(M <= INT64_MAX / (ld_x > ld_y ? ld_x : ld_y), "esc_act_fwd: M * ld overflows");
  if (act == 1) launch_act_fwd<1>(X, ld_x, M, C, Y, ld_y, (hipStream_t)stream);
  else launch_act_fwd<2>(X, ld_x, M, C, Y, ld_y, (hipStream_t)stream);
  ESC_CHECK_LAUNCH("esc_act_fwd");
  return ESC_OK;
}

int esc_act_bwd(const float* Y, int64_t ld_y, const float* dY, int64_t ld_dy, int64_t M, int64_t C, int act, float* dX,
                int64_t ld_dx, void* stream) {
  ESC_REQUIRE(act == 1 || act == 2, "esc_act_bwd: activation code %d (1 = ReLU, 2 = ELU)", act);
  ESC_REQUIRE(M >= 0 && C >= 0, "esc_act_bwd: negative size M=%ld C=%ld", (long)M, (long)C);
  ESC_REQUIRE(ld_y >= C && ld_dy >= C && ld_dx >= C, "esc_act_bwd: leading dimensions %ld / %ld / %ld below C=%ld", (long)ld_y,
              (long)ld_dy, (long)ld_dx, (long)C);
  if (M == 0 || C == 0) return ESC_OK;
  ESC_REQUIRE(Y && dY && dX, "esc_act_bwd: null pointer");
  const int64_t ld_max = ld_y > ld_dy ? (ld_y > ld_dx ? ld_y : ld_dx) : (ld_dy > ld_dx ? ld_dy : ld_dx);
  ESC_REQUIRE(M <= INT64_MAX / ld_max, "esc_act_bwd: M * ld overflows");
  if (act == 1) launch_act_bwd<1>(Y, ld_y, dY, ld_dy, M, C, dX, ld_dx, (hipStream_t)stream);
  else launch_act_bwd<2>(Y, ld_y, dY, ld_dy, M, C, dX, ld_dx, (hipStream_t)stream);
  ESC_CHECK_LAUNCH("esc_act_bwd");
  return ESC_OK;
}

}  // extern "C"
