// BiLSTM backward through time (the autograd of nn.LSTM, reached from train.py:110 loss.backward()); the forward recurrence is lstm_fwd.hip.
// Saved by the training forward: activated gates i,f,g,o [B][T][8H] and cell states [B][T][2H].
// Per step (t descending for the forward direction, ascending for the reverse one):
//   dh  = dOut[t] + W_hh^T dgates_{prev step}            <- the only sequential contraction
//   do' = dh*tanh(c)*o(1-o)          dc = dh*o*(1-tanh(c)^2) + dc_carry
//   di' = dc*g*i(1-i)   df' = dc*c_prev*f(1-f)   dg' = dc*i*(1-g^2)   dc_carry = dc*f
// The gate pre-activation gradients overwrite the saved gates in place ([B][T][8H] = dxg, the
// operand of the big dW_ih / dFeat GEMMs afterwards) and are also written in MFMA B-fragment
// order for the next step's matvec.  Workgroup = 8 waves owns 32 hidden units x 32 batch rows:
// M = units (A = W_hh^T packed in fragment order), N = batch, K = 4H gate rows split over the 8
// waves and combined through LDS; the gate math then runs on 256 threads, one (4 units, batch)
// item each, with float4 accesses along the unit axis.
#include "lstm_common.h"

namespace {

// packed W_hh^T: [dir][ut = ceil(H/32)][q = 4H/8][lane 64][4]; element j of the float4:
//   W_hh[dir][r = 8q + 2j + (lane>>5)][unit = 32*ut + (lane&31)]   (0 for unit >= H)
__global__ void lstm_pack_whh_t_kernel(const float* __restrict__ whh_f, const float* __restrict__ whh_b,
                                       float* __restrict__ wp, int H) {
  const int NUT = (H + 31) / 32, NQ = H / 2;
  const long long total = 2LL * NUT * NQ * 256;
  long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int j = idx & 3;
  const int lane = (idx >> 2) & 63;
  long long rest = idx >> 8;
  const int q = rest % NQ; rest /= NQ;
  const int ut = rest % NUT;
  const int dir = rest / NUT;
  const int r = 8 * q + 2 * j + (lane >> 5);
  const int unit = ut * 32 + (lane & 31);
  const float* w = dir ? whh_b : whh_f;
  wp[idx] = unit < H ? w[(size_t)r * H + unit] : 0.f;
}

struct LstmBwdArgs {
  const float* wpt;      // packed W_hh^T
  const float* g_prev;   // fragment-order dgates of the previous backward step: [2][NBT][NQ][64][4]
  float* g_next;
  float* gates;          // [B][T][8H]: activated gates in, pre-activation gradients out
  const float* c_all;    // [B][T][2H]
  const float* dout;     // [B][T][2H]
  float* dc;             // [2][Bpad][H] carried dc*f
  int B, T, H, Bpad, step;
};

constexpr int kBwdChunk = 13;   // K-quads per wave in flight at once

__global__ __launch_bounds__(512)
void lstm_bwd_step_kernel(LstmBwdArgs a) {
  __shared__ float sRed[8 * 16 * 64];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NQ = a.H / 2;
  const int NUT = (a.H + 31) / 32;
  const int NBT = a.Bpad / 32;
  const int ut = blockIdx.x % NUT;
  const int bt = blockIdx.x / NUT;
  const int dir = blockIdx.y;
  const int t = dir ? a.step : (a.T - 1 - a.step);
  const int tp = dir ? t + 1 : t - 1;                 // forward-order predecessor (c_{t-1})
  const bool recur = a.step > 0;

  // gate-math operands of this thread's item (waves 0..3): issued before the matvec
  const int b31 = tid & 31, ug = (tid >> 5) & 7;
  const int b = bt * 32 + b31;
  const int u0 = ut * 32 + 4 * ug;
  const bool item = tid < 256 && b < a.B && u0 < a.H;
  // (lstm_bwd_load_item's loads and the persistent kernels' gate arithmetic, written out: this kernel reads and writes the dc carry in
  // memory among them, and with the helper its instruction stream moves -- profiles/lstm_split.md)
  float4 gi4, gf4, gg4, go4, c4, cp4, dh4, dcc4;
  gi4 = gf4 = gg4 = go4 = c4 = cp4 = dh4 = dcc4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float* grow = a.gates + ((size_t)(item ? b : 0) * a.T + t) * (8 * a.H) + (size_t)dir * 4 * a.H + (item ? u0 : 0);
  float* dcp = a.dc + ((size_t)dir * a.Bpad + (item ? b : 0)) * a.H + (item ? u0 : 0);
  if (item) {
    gi4 = *reinterpret_cast<const float4*>(grow);
    gf4 = *reinterpret_cast<const float4*>(grow + a.H);
    gg4 = *reinterpret_cast<const float4*>(grow + 2 * a.H);
    go4 = *reinterpret_cast<const float4*>(grow + 3 * a.H);
    const size_t so = ((size_t)b * a.T + t) * (2 * a.H) + (size_t)dir * a.H + u0;
    c4 = *reinterpret_cast<const float4*>(a.c_all + so);
    dh4 = *reinterpret_cast<const float4*>(a.dout + so);
    if (tp >= 0 && tp < a.T)
      cp4 = *reinterpret_cast<const float4*>(a.c_all + ((size_t)b * a.T + tp) * (2 * a.H) + (size_t)dir * a.H + u0);
    if (recur) dcc4 = *reinterpret_cast<const float4*>(dcp);
  }

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (recur) {
    const float4* wq = reinterpret_cast<const float4*>(a.wpt) + ((size_t)(dir * NUT + ut) * NQ) * 64 + lane;
    const float4* gq = reinterpret_cast<const float4*>(a.g_prev) + (((size_t)dir * NBT + bt) * NQ) * 64 + lane;
    for (int base = 0; wave + 8 * base < NQ; base += kBwdChunk) {
      float4 w4[kBwdChunk], g4[kBwdChunk];
#pragma unroll
      for (int i = 0; i < kBwdChunk; ++i) {
        const int q = wave + 8 * (base + i);
        const bool ok = q < NQ;
        w4[i] = ok ? wq[(size_t)q * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
        g4[i] = ok ? gq[(size_t)q * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int i = 0; i < kBwdChunk; ++i) {
        if (wave + 8 * (base + i) < NQ) acc = lstm_mfma_quad(w4[i], g4[i], acc);      // wave-uniform
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) sRed[(wave * 16 + r) * 64 + lane] = acc[r];
  __syncthreads();
  if (tid >= 256) return;
  // item (ug, b31): D rows 4*ug..4*ug+3 live in lane (ug&1)*32 + b31 = this thread's own lane index,
  // registers 4*(ug>>1) + u with ug>>1 == this thread's wave index
  float dh[4] = {dh4.x, dh4.y, dh4.z, dh4.w};
#pragma unroll
  for (int w = 0; w < 8; ++w)
#pragma unroll
    for (int u = 0; u < 4; ++u) dh[u] += sRed[(w * 16 + 4 * wave + u) * 64 + lane];
  if (!item) return;

  const float gi[4] = {gi4.x, gi4.y, gi4.z, gi4.w}, gf[4] = {gf4.x, gf4.y, gf4.z, gf4.w};
  const float gg[4] = {gg4.x, gg4.y, gg4.z, gg4.w}, go[4] = {go4.x, go4.y, go4.z, go4.w};
  const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, cp[4] = {cp4.x, cp4.y, cp4.z, cp4.w};
  const float dcc[4] = {dcc4.x, dcc4.y, dcc4.z, dcc4.w};
  float di[4], df[4], dg[4], dO[4], dcn[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float tc = vs_tanh_fast(cc[u]);
    dO[u] = dh[u] * tc * go[u] * (1.f - go[u]);
    const float dc = fmaf(dh[u] * go[u], 1.f - tc * tc, dcc[u]);
    di[u] = dc * gg[u] * gi[u] * (1.f - gi[u]);
    df[u] = dc * cp[u] * gf[u] * (1.f - gf[u]);
    dg[u] = dc * gi[u] * (1.f - gg[u] * gg[u]);
    dcn[u] = dc * gf[u];
  }
  *reinterpret_cast<float4*>(grow) = make_float4(di[0], di[1], di[2], di[3]);
  *reinterpret_cast<float4*>(grow + a.H) = make_float4(df[0], df[1], df[2], df[3]);
  *reinterpret_cast<float4*>(grow + 2 * a.H) = make_float4(dg[0], dg[1], dg[2], dg[3]);
  *reinterpret_cast<float4*>(grow + 3 * a.H) = make_float4(dO[0], dO[1], dO[2], dO[3]);
  *reinterpret_cast<float4*>(dcp) = make_float4(dcn[0], dcn[1], dcn[2], dcn[3]);
  float* gn = a.g_next + (((size_t)dir * NBT + bt) * NQ) * 256;
#pragma unroll
  for (int gate = 0; gate < 4; ++gate) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = gate * a.H + u0 + u;
      const float v = gate == 0 ? di[u] : gate == 1 ? df[u] : gate == 2 ? dg[u] : dO[u];
      gn[((size_t)(r >> 3) * 64 + (r & 1) * 32 + b31) * 4 + ((r & 7) >> 1)] = v;
    }
  }
}


// ---------------------------------------------------------------------------------------------
// Persistent BPTT: lstm_bwd_step_kernel's decomposition and arithmetic (bit-identical results) in ONE
// launch.  Workgroup (dir, bt, ut) keeps its slice of W_hh^T (32 units x 4H rows: 25 float4 per lane
// and wave at H = 400) in registers and the dc carry in the registers of the thread that owns the
// (4 units, batch row) item; the gate gradients travel in MFMA fragment order with the same
// write-through store -> drain -> flag / flag sweep -> sc1 load hand-off as the forward recurrence
// (one flag per STORING WAVE, so no workgroup barrier sits between the stores and the flags).
// ---------------------------------------------------------------------------------------------
struct LstmBwdPersistArgs {
  const float* wpt;
  float* gbuf0;          // fragment-order gate gradients [2 dir][NBT][H/2][64][4]
  float* gbuf1;
  unsigned* flags;       // [2 dir][NBT][NUT*4]
  unsigned* err;
  float* gates;
  const float* c_all;
  const float* dout;
  int B, T, H, Bpad, bt0;
};

constexpr int kBwdResident = 25;   // K-quads of W_hh^T per wave held in registers (H <= 400); the rest streams from L2

__global__ __launch_bounds__(512)
void lstm_bwd_persistent_kernel(LstmBwdPersistArgs a) {
  __shared__ float sRed[8 * 16 * 64];
  __shared__ int sDead;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int NQ = a.H / 2;
  const int NUT = (a.H + 31) / 32;
  const int NBT = a.Bpad / 32;
  const int HQ = a.H / 8;
  const int ut = blockIdx.x % NUT;
  const int bt = a.bt0 + blockIdx.x / NUT;
  const int dir = blockIdx.y;
  if (tid == 0) sDead = 0;

  const int b31 = tid & 31, ug = (tid >> 5) & 7;
  const int b = bt * 32 + b31;
  const int u0 = ut * 32 + 4 * ug;
  const bool units_ok = tid < 256 && u0 < a.H;          // wave-uniform (H % 8 == 0)
  const bool item = units_ok && b < a.B;

  const float4* wq = reinterpret_cast<const float4*>(a.wpt) + ((size_t)(dir * NUT + ut) * NQ) * 64 + lane;
  float4 w4[kBwdResident];
#pragma unroll
  for (int i = 0; i < kBwdResident; ++i) {
    const int q = wave + 8 * i;
    w4[i] = q < NQ ? wq[(size_t)q * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const size_t group = (size_t)dir * NBT + bt;
  const unsigned gbytes = (unsigned)((size_t)2 * NBT * NQ * 64 * 16);
  __amdgpu_buffer_rsrc_t grs[2] = {__builtin_amdgcn_make_buffer_rsrc(a.gbuf0, 0, gbytes, 0x00020000),
                                   __builtin_amdgcn_make_buffer_rsrc(a.gbuf1, 0, gbytes, 0x00020000)};
  const int nflag = NUT * 4;
  unsigned* const gflags = a.flags + group * nflag;
  float dcc[4] = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();

#pragma unroll 1
  for (int s = 0; s < a.T; ++s) {
    const int t = dir ? s : (a.T - 1 - s);
    const int tp = dir ? t + 1 : t - 1;                 // forward-order predecessor (c_{t-1})
    // gate-math operands of this thread's item: independent of the exchange, issued before the wait
    float4 gi4, gf4, gg4, go4, c4, cp4, dh4;
    float* grow = lstm_bwd_load_item(gi4, gf4, gg4, go4, c4, cp4, dh4, a.gates, a.c_all, a.dout, item, b, u0, t, tp, a.T, a.H, dir);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (s > 0) {
      if (wave == 0 && !sDead) {
        unsigned spins = 0;
        for (;;) {
          bool ok = true;
          for (int j = lane; j < nflag; j += 64)
            ok = ok && (__hip_atomic_load(gflags + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned)s);
          if (__all(ok)) break;
          if (++spins > kSpinLimit) {
            lstm_give_up(lane, &sDead, a.err);
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
      }
      __syncthreads();
      const unsigned goff = (unsigned)((group * NQ * 64 + lane) * 16);
      // resident quads in register batches
      constexpr int kBatch = 9;        // loads in flight per wave (25 = 9 + 9 + 7); same MFMA order as the step kernel
#pragma unroll
      for (int base = 0; base < kBwdResident; base += kBatch) {
        u32x4_t g4[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
          const int q = wave + 8 * (base + i);
          g4[i] = (base + i < kBwdResident && q < NQ) ? __builtin_amdgcn_raw_buffer_load_b128(grs[s & 1], goff + (unsigned)q * 1024u, 0, 16 /* sc1 */)
                                                      : u32x4_t{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int i = 0; i < kBatch; ++i) {
          if (base + i < kBwdResident && wave + 8 * (base + i) < NQ)      // wave-uniform
            acc = lstm_mfma_quad(w4[base + i], lstm_as_float4(g4[i]), acc);
        }
      }
      for (int q = wave + 8 * kBwdResident; q < NQ; q += 8) {        // H > 400: weights re-read from L2 each step
        const float4 w = wq[(size_t)q * 64];
        acc = lstm_mfma_quad(w, lstm_as_float4(__builtin_amdgcn_raw_buffer_load_b128(grs[s & 1], goff + (unsigned)q * 1024u, 0, 16)), acc);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) sRed[(wave * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();
    if (tid < 256) {
      float dh[4] = {dh4.x, dh4.y, dh4.z, dh4.w};
#pragma unroll
      for (int w = 0; w < 8; ++w)
#pragma unroll
        for (int u = 0; u < 4; ++u) dh[u] += sRed[(w * 16 + 4 * wave + u) * 64 + lane];
      const float gi[4] = {gi4.x, gi4.y, gi4.z, gi4.w}, gf[4] = {gf4.x, gf4.y, gf4.z, gf4.w};
      const float gg[4] = {gg4.x, gg4.y, gg4.z, gg4.w}, go[4] = {go4.x, go4.y, go4.z, go4.w};
      const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, cp[4] = {cp4.x, cp4.y, cp4.z, cp4.w};
      float dg4[4][4];        // [gate i,f,g,o][unit]
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float tc = vs_tanh_fast(cc[u]);
        dg4[3][u] = dh[u] * tc * go[u] * (1.f - go[u]);
        const float dc = fmaf(dh[u] * go[u], 1.f - tc * tc, dcc[u]);
        dg4[0][u] = dc * gg[u] * gi[u] * (1.f - gi[u]);
        dg4[1][u] = dc * cp[u] * gf[u] * (1.f - gf[u]);
        dg4[2][u] = dc * gi[u] * (1.f - gg[u] * gg[u]);
        dcc[u] = dc * gf[u];
      }
      if (!item) {
#pragma unroll
        for (int gate = 0; gate < 4; ++gate)
#pragma unroll
          for (int u = 0; u < 4; ++u) dg4[gate][u] = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) dcc[u] = 0.f;
      }
      // fragment-order copy for the next step: quad (gate, ut, wave) = rows gate*H + ut*32 + 8*wave .. +7,
      // lane (hl, b) holds rows {hl, 2+hl, 4+hl, 6+hl}; this lane computed 4*half .. 4*half+3
      if (units_ok) {
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) {
          const float s0 = half ? dg4[gate][0] : dg4[gate][1], s1 = half ? dg4[gate][2] : dg4[gate][3];
          const float r0 = __shfl_xor(s0, 32, 64), r1 = __shfl_xor(s1, 32, 64);
          u32x4_t v;
          v[0] = __float_as_uint(half ? r0 : dg4[gate][0]);
          v[1] = __float_as_uint(half ? r1 : dg4[gate][2]);
          v[2] = __float_as_uint(half ? dg4[gate][1] : r0);
          v[3] = __float_as_uint(half ? dg4[gate][3] : r1);
          const size_t quad = group * NQ + (size_t)gate * HQ + ut * 4 + wave;
          __builtin_amdgcn_raw_buffer_store_b128(v, grs[(s + 1) & 1], (unsigned)((quad * 64 + lane) * 16), 0, 16 /* sc1 */);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_store(gflags + ut * 4 + wave, (unsigned)(s + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (item) lstm_bwd_store_grads(grow, a.H, dg4);
    }
  }
}

// bf16 form of W_hh^T for the BPTT: [dir][ut = ceil(H/32)][c = H/4][lane 64] x 16 bytes; element j:
//   W_hh[dir][r = 16c + 8*(lane>>5) + j][unit = 32*ut + (lane&31)]   (0 for unit >= H)
__global__ void lstm_pack16_t_kernel(const float* __restrict__ whh_f, const float* __restrict__ whh_b, u32x4_t* __restrict__ wp, int H) {
  const int NUT = (H + 31) / 32, NCt = H / 4;
  const long long total = 2LL * NUT * NCt * 64;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int lane = idx & 63;
  long long rest = idx >> 6;
  const int c = rest % NCt; rest /= NCt;
  const int ut = rest % NUT;
  const int dir = rest / NUT;
  const int unit = ut * 32 + (lane & 31);
  const int r0 = 16 * c + 8 * (lane >> 5);
  const float* w = dir ? whh_b : whh_f;
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (__bf16)(unit < H ? w[(size_t)(r0 + j) * H + unit] : 0.f);
  wp[idx] = __builtin_bit_cast(u32x4_t, v);
}

struct Lstm16BwdArgs {
  const u32x4_t* wpt;    // lstm_pack16_t_kernel
  void* gbuf0;           // bf16 gate gradients [2 dir][NBT][H/4][64 lane] x 16 bytes
  void* gbuf1;
  unsigned* flags;       // [2 dir][NBT][NUT*4]
  unsigned* err;
  float* gates;
  const float* c_all;
  const float* dout;
  int B, T, H, Bpad, bt0;
};

constexpr int kBwdRes16 = 13;   // 16-wide K chunks of W_hh^T per wave held in registers (4H <= 1664); the rest streams from L2

__global__ __launch_bounds__(512)
void lstm16_bwd_persistent_kernel(Lstm16BwdArgs a) {
  __shared__ float sRed[8 * 16 * 64];
  __shared__ int sDead;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int NCt = a.H / 4;
  const int NUT = (a.H + 31) / 32;
  const int NBT = a.Bpad / 32;
  const int ut = blockIdx.x % NUT;
  const int bt = a.bt0 + blockIdx.x / NUT;
  const int dir = blockIdx.y;
  if (tid == 0) sDead = 0;

  const int b31 = tid & 31, ug = (tid >> 5) & 7;
  const int b = bt * 32 + b31;
  const int u0 = ut * 32 + 4 * ug;
  const bool units_ok = tid < 256 && u0 < a.H;          // wave-uniform (H % 8 == 0)
  const bool item = units_ok && b < a.B;

  const u32x4_t* wq = a.wpt + ((size_t)(dir * NUT + ut) * NCt) * 64 + lane;
  bf16x8 w[kBwdRes16];
#pragma unroll
  for (int i = 0; i < kBwdRes16; ++i) {
    const int c = wave + 8 * i;
    w[i] = __builtin_bit_cast(bf16x8, c < NCt ? wq[(size_t)c * 64] : u32x4_t{0u, 0u, 0u, 0u});
  }
  const size_t group = (size_t)dir * NBT + bt;
  const unsigned gbytes = (unsigned)((size_t)2 * NBT * NCt * 1024);
  __amdgpu_buffer_rsrc_t grs[2] = {__builtin_amdgcn_make_buffer_rsrc(a.gbuf0, 0, gbytes, 0x00020000),
                                   __builtin_amdgcn_make_buffer_rsrc(a.gbuf1, 0, gbytes, 0x00020000)};
  const int nflag = NUT * 4;
  unsigned* const gflags = a.flags + group * nflag;
  float dcc[4] = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();

#pragma unroll 1
  for (int s = 0; s < a.T; ++s) {
    const int t = dir ? s : (a.T - 1 - s);
    const int tp = dir ? t + 1 : t - 1;                 // forward-order predecessor (c_{t-1})
    float4 gi4, gf4, gg4, go4, c4, cp4, dh4;
    float* grow = lstm_bwd_load_item(gi4, gf4, gg4, go4, c4, cp4, dh4, a.gates, a.c_all, a.dout, item, b, u0, t, tp, a.T, a.H, dir);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (s > 0) {
      if (wave == 0 && !sDead) {
        unsigned spins = 0;
        for (;;) {
          bool ok = true;
          for (int j = lane; j < nflag; j += 64)
            ok = ok && (__hip_atomic_load(gflags + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned)s);
          if (__all(ok)) break;
          if (++spins > kSpinLimit) {
            lstm_give_up(lane, &sDead, a.err);
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
      }
      __syncthreads();
      const unsigned goff = (unsigned)((group * NCt * 64 + lane) * 16);
      bf16x8 g[kBwdRes16];
#pragma unroll
      for (int i = 0; i < kBwdRes16; ++i) {
        const int c = wave + 8 * i;
        g[i] = __builtin_bit_cast(bf16x8, c < NCt ? __builtin_amdgcn_raw_buffer_load_b128(grs[s & 1], goff + (unsigned)c * 1024u, 0, 16 /* sc1 */)
                                                  : u32x4_t{0u, 0u, 0u, 0u});
      }
#pragma unroll
      for (int i = 0; i < kBwdRes16; ++i) {
        if (wave + 8 * i < NCt)        // wave-uniform
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[i], g[i], acc, 0, 0, 0);
      }
      for (int c = wave + 8 * kBwdRes16; c < NCt; c += 8) {        // H > 416: weights re-read from L2 each step
        const bf16x8 wc = __builtin_bit_cast(bf16x8, wq[(size_t)c * 64]);
        const bf16x8 gc = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(grs[s & 1], goff + (unsigned)c * 1024u, 0, 16));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wc, gc, acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) sRed[(wave * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();
    if (tid < 256) {
      float dh[4] = {dh4.x, dh4.y, dh4.z, dh4.w};
#pragma unroll
      for (int w8 = 0; w8 < 8; ++w8)
#pragma unroll
        for (int u = 0; u < 4; ++u) dh[u] += sRed[(w8 * 16 + 4 * wave + u) * 64 + lane];
      const float gi[4] = {gi4.x, gi4.y, gi4.z, gi4.w}, gf[4] = {gf4.x, gf4.y, gf4.z, gf4.w};
      const float gg[4] = {gg4.x, gg4.y, gg4.z, gg4.w}, go[4] = {go4.x, go4.y, go4.z, go4.w};
      const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, cp[4] = {cp4.x, cp4.y, cp4.z, cp4.w};
      float dg4[4][4];        // [gate i,f,g,o][unit]
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float tc = vs_tanh_fast(cc[u]);
        dg4[3][u] = dh[u] * tc * go[u] * (1.f - go[u]);
        const float dc = fmaf(dh[u] * go[u], 1.f - tc * tc, dcc[u]);
        dg4[0][u] = dc * gg[u] * gi[u] * (1.f - gi[u]);
        dg4[1][u] = dc * cp[u] * gf[u] * (1.f - gf[u]);
        dg4[2][u] = dc * gi[u] * (1.f - gg[u] * gg[u]);
        dcc[u] = dc * gf[u];
      }
      if (!item) {
#pragma unroll
        for (int gate = 0; gate < 4; ++gate)
#pragma unroll
          for (int u = 0; u < 4; ++u) dg4[gate][u] = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) dcc[u] = 0.f;
      }
      // next step's operand: rows gate*H + ut*32 + 8*wave .. +7 = one half-chunk; this lane computed 4*half .. 4*half+3 of them
      if (units_ok) {
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) {
          bf16x8 v;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float o = __shfl_xor(dg4[gate][u], 32, 64);
            v[u] = (__bf16)(half ? o : dg4[gate][u]);
            v[4 + u] = (__bf16)(half ? dg4[gate][u] : o);
          }
          const int r0 = gate * a.H + ut * 32 + 8 * wave;
          const unsigned off = (unsigned)(((group * NCt + (r0 >> 4)) * 64 + ((r0 >> 3) & 1) * 32 + b31) * 16);
          if (half == 0)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), grs[(s + 1) & 1], off, 0, 16 /* sc1 */);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_store(gflags + ut * 4 + wave, (unsigned)(s + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (item) lstm_bwd_store_grads(grow, a.H, dg4);
    }
  }
}

}  // namespace

// W_hh^T in fp32 fragment form, then room for the bf16 form (VS_MATH_BF16's BPTT), then 64 spare floats
static size_t lstm_packed_t_fp32_floats(int H) { return (size_t)2 * ((H + 31) / 32) * (H / 2) * 256; }
static size_t lstm_packed_t_bf16_floats(int H) { return (size_t)2 * ((H + 31) / 32) * (H / 4) * 256; }
extern "C" size_t vs_lstm_packed_t_floats(int H) { return lstm_packed_t_fp32_floats(H) + lstm_packed_t_bf16_floats(H) + 64; }
// backward state: dgates fragments ping/pong [2][2][NBT][H/2][256] + dc carry [2][Bpad][H]
extern "C" size_t vs_lstm_bwd_state_floats(int B, int H) {
  const size_t Bpad = ((size_t)B + 31) / 32 * 32;
  return 2 * (2 * (Bpad / 32) * (size_t)(H / 2) * 256) + 2 * Bpad * H + 64;   // + 64: error word of the persistent kernel
}

int vs_lstm_pack_t_impl(const float* whh_f, const float* whh_b, float* wp, int H, hipStream_t stream, int math) {
  VS_REQUIRE(H > 0 && H % 8 == 0, "lstm: hidden size %d must be a multiple of 8", H);
  const long long total = (long long)lstm_packed_t_fp32_floats(H);
  hipLaunchKernelGGL(lstm_pack_whh_t_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, whh_f, whh_b, wp, H);
  VS_LAUNCH_CHECK();
  if (math != VS_MATH_CODE_BF16) return 0;
  const long long slots = 2LL * ((H + 31) / 32) * (H / 4) * 64;
  hipLaunchKernelGGL(lstm_pack16_t_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, whh_f, whh_b,
                     reinterpret_cast<u32x4_t*>(wp + lstm_packed_t_fp32_floats(H)), H);
  VS_LAUNCH_CHECK();
  return 0;
}

// gates: activated gates from the training forward, overwritten with d(loss)/d(gate pre-activations).
// state: step kernels = dgates fragments ping/pong + dc carry; persistent kernel = the two fragment
// buffers, then (in the dc region) the flag words and the error word.
int vs_bilstm_bwd_recurrent_impl(const float* wpt, float* state, float* gates, const float* c_all, const float* dout,
                                 int B, int T, int H, hipStream_t stream, int math) {
  VS_REQUIRE(B > 0 && T > 0 && H > 0 && H % 8 == 0, "lstm_bwd: bad shape B=%d T=%d H=%d (H must be a multiple of 8)", B, T, H);
  const int mode = vs_lstm_kernel_mode();
  if (mode == 3) math = VS_MATH_CODE_FP32;
  const int Bpad = (B + 31) / 32 * 32;
  const size_t frag = (size_t)2 * (Bpad / 32) * (H / 2) * 256;
  VS_CHECK_HIP(hipMemsetAsync(state, 0, vs_lstm_bwd_state_floats(B, H) * sizeof(float), stream));
  float* gbuf[2] = {state, state + frag};
  const int NUT = (H + 31) / 32, NBT = Bpad / 32;
  int bt_per_launch = 0, cus = 0;
  if (int rc = lstm_tiles_per_launch(2 * NUT, &bt_per_launch, &cus)) return rc;
  const bool persistent = mode != 1 && bt_per_launch >= 1;
  VS_REQUIRE(mode != 2 || persistent, "lstm_bwd: persistent recurrence needs %d workgroups <= %d CUs", 2 * NUT, cus);
  // (the tagged-data hand-off of the forward recurrence was built for this kernel too in round 5: correct and 5 % slower -- eight waves
  // poll 13 KB each per round -- so the BPTT keeps its flags: tools/attic/lstm16_bwd_tagged_kernel.hip.txt)
  if (persistent) {
    unsigned* flags = reinterpret_cast<unsigned*>(state + 2 * frag);      // 2*Bpad*H words available, 2*NBT*NUT*4 used
    unsigned* err = reinterpret_cast<unsigned*>(state + 2 * frag + (size_t)2 * Bpad * H);
    bool launched = true;
    for (int bt0 = 0; bt0 < NBT; bt0 += bt_per_launch) {
      const int nbt = NBT - bt0 < bt_per_launch ? NBT - bt0 : bt_per_launch;
      hipError_t e;
      if (math == VS_MATH_CODE_BF16) {      // gate gradients and W_hh^T as bf16 (the fragment buffers are half as large)
        Lstm16BwdArgs a{reinterpret_cast<const u32x4_t*>(wpt + lstm_packed_t_fp32_floats(H)), gbuf[0], gbuf[1], flags, err, gates, c_all, dout,
                        B, T, H, Bpad, bt0};
        e = launch_resident(reinterpret_cast<const void*>(&lstm16_bwd_persistent_kernel), dim3(NUT * nbt, 2), dim3(512), a, stream);
      } else {
        LstmBwdPersistArgs a{wpt, gbuf[0], gbuf[1], flags, err, gates, c_all, dout, B, T, H, Bpad, bt0};
        e = launch_resident(reinterpret_cast<const void*>(&lstm_bwd_persistent_kernel), dim3(NUT * nbt, 2), dim3(512), a, stream);
      }
      if (e != hipSuccess) {
        (void)hipGetLastError();
        VS_REQUIRE(bt0 == 0 && mode != 2, "lstm_bwd: persistent recurrence could not be launched resident: %s", hipGetErrorString(e));
        launched = false;
        break;
      }
    }
    if (launched) return vs_lstm_poison_impl(err, gates, (long long)B * T * 8 * H, stream);
  }
  if (persistent) VS_CHECK_HIP(hipMemsetAsync(state, 0, vs_lstm_bwd_state_floats(B, H) * sizeof(float), stream));
  float* dc = state + 2 * frag;
  dim3 grid(NUT * NBT, 2), block(512);
  for (int s = 0; s < T; ++s) {
    LstmBwdArgs a{wpt, gbuf[s & 1], gbuf[(s + 1) & 1], gates, c_all, dout, dc, B, T, H, Bpad, s};
    hipLaunchKernelGGL(lstm_bwd_step_kernel, grid, block, 0, stream, a);
  }
  VS_LAUNCH_CHECK();
  return 0;
}
