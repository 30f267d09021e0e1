// What lstm_fwd.hip and lstm_bwd.hip share: the operand types and constants of the persistent recurrences, the pieces of device code
// their kernels have in common, and the launchers' residency arithmetic.  Every helper is inlined, and the rule of this header is that
// a kernel calls one only where its instruction stream stays the one it had with the code written out (profiles/lstm_split.md lists
// the call sites that keep a written-out copy for that reason; each says so in a comment and has to be kept in step with this file).
#pragma once
#include "vs_internal.h"

namespace {

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr unsigned kSpinLimit = 1u << 22;      // flag sweeps / poll rounds before a persistent kernel gives up
constexpr float kHScale = 1024.f;              // h of the split form is exchanged as f16(h * 2^10)
constexpr int kMaxC = 7;                       // 16-wide K chunks per wave held in registers by the f16 forward kernels (H <= 448)
constexpr unsigned kSentinel = 0x7FFF7FFFu;    // an unwritten slot of the tagged-data hand-off: two 16-bit NaNs in every dword
constexpr unsigned kUnSentinel = 0x7FFF7E00u;  // what a computed dword of that pattern is stored as: NaN still, not the sentinel

// ---- forward: wave 0's epilogue ---------------------------------------------------------------------------------------------------------

// The 16 gate values of this lane's (4 units, batch column) in row `row` of a [rows][8H] array: where they start ...
__device__ __forceinline__ const float* lstm_gate_row(const float* base, size_t row, int dir, int jg, int half, int H) {
  return base + row * (8 * H) + (size_t)dir * 4 * H + jg * 8 + 4 * half;
}
// ... and value r = 4*gate + u: unit jg*8 + 4*half + u of gate `gate`.  ok = false (padding column): zero, nothing is read.
// (The callers loop over r themselves: a helper that fills the array merges the 16 guarded loads and moves every forward stream.)
__device__ __forceinline__ float lstm_gate_at(const float* xrow, int r, int H, bool ok) { return ok ? xrow[(r >> 2) * H + (r & 3)] : 0.f; }

// One LSTM cell step of unit u of this lane's 4: gate pre-activations acc + xg (SCALED: acc * inv + xg, the f16 products' accumulator
// scale), c = f*c + i*g, h = o*tanh(c); cprev advances.
template <bool SCALED>
__device__ __forceinline__ void lstm_cell_unit(int u, const f32x16& acc, float inv, const float (&xgv)[16], float (&cprev)[4], float (&hv)[4],
                                               float (&cnew)[4], float (&gact)[4][4]) {
  const float gi = vs_sigmoid_fast(SCALED ? fmaf(acc[0 + u], inv, xgv[0 + u]) : acc[0 + u] + xgv[0 + u]);
  const float gf = vs_sigmoid_fast(SCALED ? fmaf(acc[4 + u], inv, xgv[4 + u]) : acc[4 + u] + xgv[4 + u]);
  const float gg = vs_tanh_fast(SCALED ? fmaf(acc[8 + u], inv, xgv[8 + u]) : acc[8 + u] + xgv[8 + u]);
  const float go = vs_sigmoid_fast(SCALED ? fmaf(acc[12 + u], inv, xgv[12 + u]) : acc[12 + u] + xgv[12 + u]);
  const float cn = gf * cprev[u] + gi * gg;
  hv[u] = go * vs_tanh_fast(cn);
  cnew[u] = cn;
  cprev[u] = cn;
  gact[0][u] = gi; gact[1][u] = gf; gact[2][u] = gg; gact[3][u] = go;
}
// This lane's stores of one step, b < B: h to out [B][T][2H] ...
__device__ __forceinline__ void lstm_store_h(float* out, int b, int t, int T, int H, int dir, int jg, int half, const float (&hv)[4]) {
  float4* o = reinterpret_cast<float4*>(out + ((size_t)b * T + t) * (2 * H) + (size_t)dir * H + jg * 8 + 4 * half);
  *o = make_float4(hv[0], hv[1], hv[2], hv[3]);
}
// ... and, in training, the tape: c_save [B][T][2H], gates_save [B][T][8H] (activated i, f, g, o)
__device__ __forceinline__ void lstm_store_tape(float* c_save, float* gates_save, int b, int t, int T, int H, int dir, int jg, int half,
                                                const float (&cnew)[4], const float (&gact)[4][4]) {
  if (c_save) {
    float4* cs = reinterpret_cast<float4*>(c_save + ((size_t)b * T + t) * (2 * H) + (size_t)dir * H + jg * 8 + 4 * half);
    *cs = make_float4(cnew[0], cnew[1], cnew[2], cnew[3]);
  }
  if (gates_save) {
    float* grow = gates_save + ((size_t)b * T + t) * (8 * H) + (size_t)dir * 4 * H + jg * 8 + 4 * half;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq)
      *reinterpret_cast<float4*>(grow + gq * H) = make_float4(gact[gq][0], gact[gq][1], gact[gq][2], gact[gq][3]);
  }
}
// both, behind the b < B guard (the carry form of the tagged kernel puts its state hand-out between the two)
__device__ __forceinline__ void lstm_store_outputs(float* out, float* c_save, float* gates_save, int b, int B, int t, int T, int H, int dir, int jg,
                                                   int half, const float (&hv)[4], const float (&cnew)[4], const float (&gact)[4][4]) {
  if (b < B) {
    lstm_store_h(out, b, t, T, H, dir, jg, half, hv);
    lstm_store_tape(c_save, gates_save, b, t, T, H, dir, jg, half, cnew, gact);
  }
}

// ---- hand-off forms ---------------------------------------------------------------------------------------------------------------------

// f16 forward hand-off: this lane computed units 4*half .. 4*half+3 of the owner's 8 for its batch column; after the half-wave exchange
// every lane holds all 8 = one half-chunk of its column
__device__ __forceinline__ void lstm_gather_half_chunk(float (&full)[8], const float (&x)[4], int half) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float o = __shfl_xor(x[u], 32, 64);
    full[u] = half ? o : x[u];
    full[4 + u] = half ? x[u] : o;
  }
}

// The 8 values of a half-chunk of h as the f16 forward recurrence exchanges them: NP = 1 one plane, rounded to f16; NP = 2 plane 0 =
// hi = rtz f16 of h * 2^10, plane 1 = lo = rtz f16 of the remainder.  GUARD (the tagged-data hand-off): a diverged step (h = NaN with
// an all-ones payload in both halves) must not look like an unwritten slot: the consumers would spin to their bound and report "gave
// up" instead of carrying the NaN to the loss guard.  The flag hand-off has no sentinel and no guard.
template <int NP, bool GUARD>
__device__ __forceinline__ u32x4_t lstm16_pack_h(const float (&full)[8], int plane) {
  u32x4_t v;
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (NP == 2) {
      const float x0 = full[2 * j] * kHScale, x1 = full[2 * j + 1] * kHScale;
      const h2 hh = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_pkrtz(x0, x1));
      const unsigned lo = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(x0 - (float)hh[0], x1 - (float)hh[1]));
      v[j] = plane ? lo : __builtin_bit_cast(unsigned, hh);
    } else {
      const h2 hh = {(_Float16)full[2 * j], (_Float16)full[2 * j + 1]};
      v[j] = __builtin_bit_cast(unsigned, hh);
    }
    if (GUARD) v[j] = v[j] == kSentinel ? kUnSentinel : v[j];
  }
  return v;
}

// ---- matrix products --------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float4 lstm_as_float4(u32x4_t v) {
  return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}

// one K-quad (8 of K) of the fp32 recurrences
__device__ __forceinline__ f32x16 lstm_mfma_quad(const float4& w, const float4& x, f32x16 acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, x.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, x.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, x.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, x.w, acc, 0, 0, 0);
  return acc;
}

// chunk c, plane p of the f16 W_hh slice at wq (this lane's 16 bytes); zeros beyond the last chunk
template <int NP>
__device__ __forceinline__ f16x8 lstm16_load_w(const u32x4_t* wq, int c, int p, int NC) {
  return __builtin_bit_cast(f16x8, c < NC ? wq[(size_t)(c * NP + p) * 64] : u32x4_t{0u, 0u, 0u, 0u});
}

// one 16-wide K chunk of the f16 forward recurrences: NP = 2 is lo*hi + hi*lo + hi*hi (plane 0 = hi), the lo*lo term dropped
template <int NP>
__device__ __forceinline__ f32x16 lstm16_mfma_chunk(const f16x8 (&w)[NP], const f16x8 (&h)[NP], f32x16 acc) {
  if (NP == 2) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[NP - 1], h[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[0], h[NP - 1], acc, 0, 0, 0);
  }
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(w[0], h[0], acc, 0, 0, 0);
}

// ---- BPTT: one (4 units, batch row) item ----------------------------------------------------------------------------------------------

// The operands of item (b, units u0 .. u0+3) at frame t (tp: its forward-order predecessor): saved gates, c_t, c_{t-1}, dOut[t]; zeros
// when !item.  Returns the item's row of gates [B][T][8H], where the gate gradients go.  (Seven float4 and reference parameters: with a
// struct of float4, or with the scalars passed by value, the persistent kernels' streams move.)
__device__ __forceinline__ float* lstm_bwd_load_item(float4& gi4, float4& gf4, float4& gg4, float4& go4, float4& c4, float4& cp4, float4& dh4,
                                                     float* const& gates, const float* const& c_all, const float* const& dout, const bool& item,
                                                     const int& b, const int& u0, const int& t, const int& tp, const int& T, const int& H,
                                                     const int& dir) {
  gi4 = gf4 = gg4 = go4 = c4 = cp4 = dh4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float* grow = gates + ((size_t)(item ? b : 0) * T + t) * (8 * H) + (size_t)dir * 4 * H + (item ? u0 : 0);
  if (item) {
    gi4 = *reinterpret_cast<const float4*>(grow);
    gf4 = *reinterpret_cast<const float4*>(grow + H);
    gg4 = *reinterpret_cast<const float4*>(grow + 2 * H);
    go4 = *reinterpret_cast<const float4*>(grow + 3 * H);
    const size_t so = ((size_t)b * T + t) * (2 * H) + (size_t)dir * H + u0;
    c4 = *reinterpret_cast<const float4*>(c_all + so);
    dh4 = *reinterpret_cast<const float4*>(dout + so);
    if (tp >= 0 && tp < T)
      cp4 = *reinterpret_cast<const float4*>(c_all + ((size_t)b * T + tp) * (2 * H) + (size_t)dir * H + u0);
  }
  return grow;
}

// the batched GEMMs' operand, in place of the saved gates
__device__ __forceinline__ void lstm_bwd_store_grads(float* grow, int H, const float (&dg4)[4][4]) {
#pragma unroll
  for (int gate = 0; gate < 4; ++gate)
    *reinterpret_cast<float4*>(grow + gate * H) = make_float4(dg4[gate][0], dg4[gate][1], dg4[gate][2], dg4[gate][3]);
}

// ---- waiting ----------------------------------------------------------------------------------------------------------------------------

// a spin ran into its bound: the workgroup stops waiting (dead) and the launch reports through *err
__device__ __forceinline__ void lstm_give_up(int lane, int* dead, unsigned* err) {
  if (lane == 0) { *dead = 1; __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------

// Cooperative launch: the runtime checks the grid against the kernel's occupancy and refuses (instead of queueing
// workgroups behind resident ones, where the flag protocol would spin until its bound) when it cannot be resident.
template <class Args>
hipError_t launch_resident(const void* kernel, dim3 grid, dim3 block, Args& a, hipStream_t stream) {
  void* params[] = {&a};
  return hipLaunchCooperativeKernel(kernel, grid, block, params, 0, stream);
}

// One workgroup per CU at most: every workgroup of a persistent launch must be resident for its hand-off protocol.  Batch tiles one launch
// can take when a tile needs wgs_per_tile workgroups (0: not even one, the per-step kernels run); *cus: the device's CU count, for messages
inline int lstm_tiles_per_launch(int wgs_per_tile, int* tiles, int* cus) {
  int dev = 0;
  VS_CHECK_HIP(hipGetDevice(&dev));
  VS_CHECK_HIP(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
  *tiles = *cus / wgs_per_tile;
  return 0;
}

}  // namespace
