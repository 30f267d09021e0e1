// BiLSTM recurrence (the 301 sequential steps of nn.LSTM, models/voicesplit/model.py:57-61,82).
//
// The input projection x_t @ W_ih^T + b_ih + b_hh (+ d-vector fold) for every t and both
// directions is one big GEMM done beforehand (gemm_mfma.hip) into
//   xg[b][t][dir*4H + gate*H + j]          gate order i, f, g, o  (PyTorch)
// What is left per time step and direction is gates = xg_t + h_{t-1} @ W_hh^T followed by
//   c = sigmoid(f)*c + sigmoid(i)*tanh(g);   h = sigmoid(o)*tanh(c)
//
// One launch per time step (both directions, grid.y = dir); the kernel boundary is the
// device-wide dependency between steps.  Workgroup = 4 waves owns 8 hidden units x 32 batch
// rows: the 32x32 MFMA tile has rows i = 8*gate + unit and columns = batch, so after the
// K reduction each lane holds i,f,g,o of the same (unit, batch) in its own accumulator
// registers (D row = (r&3) + 8*(r>>2) + 4*(lane>>5): r>>2 = gate, (r&3)+4*(lane>>5) = unit) and
// the gate math needs no cross-lane traffic.  The K = H reduction is split over the 4 waves and
// combined through LDS.  W_hh and h are both kept in MFMA fragment order (one coalesced dwordx4
// per lane per 4 K-steps) and every load of a step is issued before its first MFMA, so a step
// costs one L2 round trip + 13 x 4 MFMAs per wave; c stays [dir][H][Bpad].
#include "lstm_common.h"

namespace {

// packed recurrent weights: [dir][jg = H/8][q = H/8][lane 64][4]; element j of the float4:
//   W_hh[dir][(i>>3)*H + jg*8 + (i&7)][8q + 2j + (lane>>5)],  i = lane & 31
__global__ void lstm_pack_whh_kernel(const float* __restrict__ whh_f, const float* __restrict__ whh_b,
                                     float* __restrict__ wp, int H) {
  const int HQ = H / 8;
  const long long total = 2LL * HQ * HQ * 256;
  long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int j = idx & 3;
  const int lane = (idx >> 2) & 63;
  long long rest = idx >> 8;
  const int q = rest % HQ; rest /= HQ;
  const int jg = rest % HQ;
  const int dir = rest / HQ;
  const int i = lane & 31;
  const int row = (i >> 3) * H + jg * 8 + (i & 7);
  const int k = 8 * q + 2 * j + (lane >> 5);
  const float* w = dir ? whh_b : whh_f;
  wp[idx] = w[(size_t)row * H + k];
}

struct LstmStepArgs {
  const float* xg;      // [B][T][8H]
  const float* wp;      // packed W_hh
  const float* h_prev;  // fragment order [2 dir][Bpad/32][H/8][64 lane][4]
  float* h_next;        // same layout
  float* c;             // [2][H][Bpad]  (updated in place: each (unit,batch) has one owner)
  float* out;           // [B][T][2H]
  float* gates_save;    // training: [B][T][8H] activated gates i,f,g,o (may alias xg), else null
  float* c_save;        // training: [B][T][2H] cell state c_t, else null
  int B, T, H, Bpad, step;
};

// h is kept in MFMA B-fragment order so a K-quad is ONE coalesced dwordx4 per lane:
//   hfrag[dir][bt][q][lane][j] = h[dir][k = 8q + 2j + (lane>>5)][b = 32*bt + (lane&31)]
__device__ __forceinline__ size_t hfrag_index(int dir, int nbt, int bt, int hq, int k, int b31) {
  const int q = k >> 3, j = (k & 7) >> 1, half = k & 1;
  return ((((size_t)dir * nbt + bt) * hq + q) * 64 + half * 32 + b31) * 4 + j;
}

constexpr int kMaxQ = 13;   // K-quads per wave held in flight at once (H <= 416 in one pass)

__global__ __launch_bounds__(256)
void lstm_step_kernel(LstmStepArgs a) {
  __shared__ float sRed[3 * 16 * 64];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int HQ = a.H / 8;
  const int NBT = a.Bpad / 32;
  const int jg = blockIdx.x % HQ;
  const int bt = blockIdx.x / HQ;
  const int dir = blockIdx.y;
  const int t = dir ? (a.T - 1 - a.step) : a.step;
  const int b = bt * 32 + l31;
  const size_t hb = (size_t)dir * a.H * a.Bpad;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  // every load of this step is issued before the first MFMA: one L2 round trip, not 13
  const float4* wq = reinterpret_cast<const float4*>(a.wp) + ((size_t)(dir * HQ + jg) * HQ) * 64 + lane;
  const float4* hq = reinterpret_cast<const float4*>(a.h_prev) + (((size_t)dir * NBT + bt) * HQ) * 64 + lane;
  const bool recur = a.step > 0;      // h_{-1} = 0: nothing to multiply at the first step
  float4 w4[kMaxQ], h4[kMaxQ];
#pragma unroll
  for (int i = 0; i < kMaxQ; ++i) {
    const int q = wave + 4 * i;
    const bool ok = recur && q < HQ;
    w4[i] = ok ? wq[(size_t)q * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
    h4[i] = ok ? hq[(size_t)q * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // wave 0 owns the epilogue: its xg / c reads travel with the operand loads
  float xgv[16], cprev[4];
  if (wave == 0) {
    const bool ok = b < a.B;
    const float* xrow = lstm_gate_row(a.xg, (size_t)(ok ? b : 0) * a.T + t, dir, jg, half, a.H);
#pragma unroll
    for (int r = 0; r < 16; ++r) xgv[r] = lstm_gate_at(xrow, r, a.H, ok);
#pragma unroll
    for (int u = 0; u < 4; ++u) cprev[u] = a.c[hb + (size_t)(jg * 8 + 4 * half + u) * a.Bpad + b];
  }
  if (recur) {
#pragma unroll
    for (int i = 0; i < kMaxQ; ++i) {
      if (wave + 4 * i < HQ) {          // wave-uniform  (lstm_mfma_quad written out, here and below: as calls they move this kernel's stream)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w4[i].x, h4[i].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w4[i].y, h4[i].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w4[i].z, h4[i].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w4[i].w, h4[i].w, acc, 0, 0, 0);
      }
    }
    // hidden sizes beyond 4*kMaxQ*8 = 416: remaining quads, plain loop
    for (int q = wave + 4 * kMaxQ; q < HQ; q += 4) {
      const float4 w = wq[(size_t)q * 64], h = hq[(size_t)q * 64];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, h.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, h.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, h.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, h.w, acc, 0, 0, 0);
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sRed[((wave - 1) * 16 + r) * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int w = 0; w < 3; ++w)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += sRed[(w * 16 + r) * 64 + lane];

  float hv[4], cnew[4], gact[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    lstm_cell_unit<false>(u, acc, 1.f, xgv, cprev, hv, cnew, gact);
    const int k = jg * 8 + 4 * half + u;
    a.c[hb + (size_t)k * a.Bpad + b] = cnew[u];   // padded batch columns only ever hold their own garbage
    a.h_next[hfrag_index(dir, NBT, bt, HQ, k, l31)] = hv[u];
  }
  lstm_store_outputs(a.out, a.c_save, a.gates_save, b, a.B, t, a.T, a.H, dir, jg, half, hv, cnew, gact);
}


// ---------------------------------------------------------------------------------------------
// Persistent form of the recurrence: ONE launch for all T steps (north_star: "persistent-RNN style
// kernel"; SURVEY.md 0.5: W_hh is 2.56 MB per direction, so it is partitioned over the CUs and the
// hidden state is exchanged once per step).
//
// Same decomposition and arithmetic as lstm_step_kernel (bit-identical results): workgroup (dir, bt,
// jg) owns 8 hidden units x 32 batch rows for the whole sequence.  What the launch boundary used to
// provide is now explicit:
//  * this workgroup's slice of W_hh (32 gate rows x H) is loaded ONCE and stays in registers
//    (13 float4 per lane and wave at H = 400), c stays in the registers of wave 0;
//  * h travels through L2 in MFMA fragment order: the owner stores its 1 KB quad write-through
//    (sc1), drains its store queue, then raises its own flag word to step+1; a consumer sweeps the
//    H/8 flag words of its (dir, batch tile) group with one relaxed agent-scope load per lane until
//    all carry the epoch, and then reads the quads with sc1 loads (L1-bypassing: the hand-off form
//    of cdna_hip_programming.md Guideline 16 R1 that needs no acquire fence) -- no atomics, no
//    counter serialisation, 50 producers <-> 50 consumers per group, groups never wait for each other;
//  * ping-pong buffers: a workgroup can only overwrite h_{s-1} after every member of its group has
//    published step s, i.e. has finished reading it.
// All workgroups of a launch must be co-resident (grid <= number of CUs, checked by the launcher,
// which otherwise walks the batch tiles in several launches); every spin is bounded and reports
// through *err instead of hanging.
// ---------------------------------------------------------------------------------------------
struct LstmPersistArgs {
  const float* xg;
  const float* wp;
  float* hbuf0;         // fragment order [2 dir][NBT][H/8][64 lane][4]
  float* hbuf1;
  unsigned* flags;      // [2 dir][NBT][H/8] epoch words, zeroed by the launcher before every launch
  unsigned* err;        // set to 1 when a spin gave up
  float* out;
  float* gates_save;
  float* c_save;
  int B, T, H, Bpad, bt0;
};

__global__ __launch_bounds__(256)
void lstm_persistent_kernel(LstmPersistArgs a) {
  __shared__ float sRed[3 * 16 * 64];
  __shared__ int sDead;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int HQ = a.H / 8;
  const int NBT = a.Bpad / 32;
  const int jg = blockIdx.x % HQ;
  const int bt = a.bt0 + blockIdx.x / HQ;
  const int dir = blockIdx.y;
  const int b = bt * 32 + l31;
  if (tid == 0) sDead = 0;

  // W_hh slice: resident for the whole sequence
  const float4* wq = reinterpret_cast<const float4*>(a.wp) + ((size_t)(dir * HQ + jg) * HQ) * 64 + lane;
  float4 w4[kMaxQ];
#pragma unroll
  for (int i = 0; i < kMaxQ; ++i) {
    const int q = wave + 4 * i;
    w4[i] = q < HQ ? wq[(size_t)q * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const size_t group = ((size_t)dir * NBT + bt) * HQ;                     // first quad / flag of this (dir, bt) group
  const unsigned hbytes = (unsigned)((size_t)2 * NBT * HQ * 64 * 16);
  __amdgpu_buffer_rsrc_t hrs[2] = {__builtin_amdgcn_make_buffer_rsrc(a.hbuf0, 0, hbytes, 0x00020000),
                                   __builtin_amdgcn_make_buffer_rsrc(a.hbuf1, 0, hbytes, 0x00020000)};
  unsigned* const gflags = a.flags + group;
  float cprev[4] = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();

#pragma unroll 1
  for (int s = 0; s < a.T; ++s) {
    const int t = dir ? (a.T - 1 - s) : s;
    // wave 0 owns the epilogue: its xg reads do not depend on h and go out before the wait
    float xgv[16];
    if (wave == 0) {
      const bool ok = b < a.B;
      const float* xrow = lstm_gate_row(a.xg, (size_t)(ok ? b : 0) * a.T + t, dir, jg, half, a.H);
#pragma unroll
      for (int r = 0; r < 16; ++r) xgv[r] = lstm_gate_at(xrow, r, a.H, ok);
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (s > 0) {
      if (wave == 0 && !sDead) {
        // every producer of this group has published h_{s-1} (epoch s)
        unsigned spins = 0;
        for (;;) {
          bool ok = true;
          for (int j = lane; j < HQ; j += 64)
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
      const unsigned hoff = (unsigned)((group * 64 + lane) * 16);
      float4 h4[kMaxQ];
#pragma unroll
      for (int i = 0; i < kMaxQ; ++i) {
        const int q = wave + 4 * i;
        h4[i] = lstm_as_float4(q < HQ ? __builtin_amdgcn_raw_buffer_load_b128(hrs[s & 1], hoff + (unsigned)q * 1024u, 0, 16 /* sc1 */)
                                      : u32x4_t{0u, 0u, 0u, 0u});
      }
#pragma unroll
      for (int i = 0; i < kMaxQ; ++i) {
        if (wave + 4 * i < HQ) acc = lstm_mfma_quad(w4[i], h4[i], acc);          // wave-uniform
      }
      // hidden sizes beyond 4*kMaxQ*8 = 416: remaining quads, weights re-read from L2 each step
      for (int q = wave + 4 * kMaxQ; q < HQ; q += 4) {
        const float4 w = wq[(size_t)q * 64];
        acc = lstm_mfma_quad(w, lstm_as_float4(__builtin_amdgcn_raw_buffer_load_b128(hrs[s & 1], hoff + (unsigned)q * 1024u, 0, 16)), acc);
      }
    }
    if (wave > 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sRed[((wave - 1) * 16 + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int w = 0; w < 3; ++w)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += sRed[(w * 16 + r) * 64 + lane];
      float hv[4], cnew[4], gact[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) lstm_cell_unit<false>(u, acc, 1.f, xgv, cprev, hv, cnew, gact);
      // h quad jg in fragment order: lane (hl, b) holds units {hl, 2+hl, 4+hl, 6+hl} of this workgroup's
      // 8; this lane computed units 4*half .. 4*half+3 -> two values come from the other half-wave
      {
        const float s0 = half ? hv[0] : hv[1], s1 = half ? hv[2] : hv[3];
        const float r0 = __shfl_xor(s0, 32, 64), r1 = __shfl_xor(s1, 32, 64);
        u32x4_t v;
        v[0] = __float_as_uint(half ? r0 : hv[0]);
        v[1] = __float_as_uint(half ? r1 : hv[2]);
        v[2] = __float_as_uint(half ? hv[1] : r0);
        v[3] = __float_as_uint(half ? hv[3] : r1);
        __builtin_amdgcn_raw_buffer_store_b128(v, hrs[(s + 1) & 1], (unsigned)(((group + jg) * 64 + lane) * 16), 0, 16 /* sc1: write-through */);
      }
      // publish: the quad has left this wave's store queue, then the flag (one lane).  The
      // outputs below are off the step-to-step critical path and go out after the flag
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_store(gflags + jg, (unsigned)(s + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      lstm_store_outputs(a.out, a.c_save, a.gates_save, b, a.B, t, a.T, a.H, dir, jg, half, hv, cnew, gact);
    }
  }
}


// ---------------------------------------------------------------------------------------------
// The recurrent products on the f16 / bf16 matrix instructions (dims.math = VS_MATH_F16X3 / VS_MATH_BF16).
//
// v_mfma_f32_32x32x2_f32 retires 2 of K per 64 cycles, v_mfma_f32_32x32x16_{f16,bf16} 16 per 32: the 52 fp32 MFMAs a
// wave issues per forward step (100 per BPTT step) are 1.5 us (3 us) of a 6.8 us (12.4 us) step whose other parts are
// hand-off latency.  Same decomposition, flags and hand-off protocol as the kernels above; what changes is the operand
// form of the exchanged vector and of the resident weights:
//   * K runs in chunks of 16; lane (half, n) of a chunk holds k = 16c + 8*half + j, j = 0..7, as ONE 16-byte vector
//     (A: rows = n, B: columns = n -- the same map on both sides, so the dot product is the plain one);
//   * forward, NP = 1 (VS_MATH_BF16): h and W_hh rounded to f16 (11 significant bits; |h| < 1, no range problem) -- one
//     product per chunk.  NP = 2 (VS_MATH_F16X3): both split into f16 hi + lo planes (h scaled by 2^10, W_hh by the
//     power of two that puts max|W_hh| into [2^9, 2^10)), three products per chunk, the 2^-22 lo x lo term dropped:
//     fp32-class, as in the split-f16 convs and GEMMs;
//   * BPTT (VS_MATH_BF16 only): gate gradients and W_hh^T as bf16 -- gradients have no a-priori range, so the 8-bit
//     exponent is the right 16-bit form; one product per chunk.  The fp32-class arithmetic keeps the fp32 MFMA BPTT.
// A producer owns 8 consecutive k (8 hidden units / 8 gate rows x 32 batch columns) = exactly one half-chunk: after a
// half-wave exchange each lane holds its column's 8 values, the lower half-wave stores the hi plane (16 B per lane),
// the upper one the lo plane.  The exchange shrinks from 4 to 2 (x NP) bytes per value.
// ---------------------------------------------------------------------------------------------

// f16 forms of W_hh for the forward recurrence: [dir][jg = H/8][c = ceil(H/16)][p < NP][lane 64] x 16 bytes; element j:
//   W_hh[dir][(i>>3)*H + jg*8 + (i&7)][16c + 8*(lane>>5) + j] * s,  i = lane & 31   (0 beyond H)
// hdr: [1] = s (NP = 2: from vs_scale_from_absmax_impl; NP = 1: unused) -> [0] = what the accumulators are multiplied by
template <int NP>
__global__ void lstm_pack16_kernel(const float* __restrict__ whh_f, const float* __restrict__ whh_b, u32x4_t* __restrict__ wp,
                                   float* __restrict__ hdr, int H) {
  const int HQ = H / 8, NC = (H + 15) / 16;
  const long long total = 2LL * HQ * NC * 64;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const float s = NP == 2 ? hdr[1] : 1.f;
  if (idx == 0) hdr[0] = NP == 2 ? hdr[2] * (1.f / kHScale) : 1.f;
  if (idx >= total) return;
  const int lane = idx & 63;
  long long rest = idx >> 6;
  const int c = rest % NC; rest /= NC;
  const int jg = rest % HQ;
  const int dir = rest / HQ;
  const int i = lane & 31;
  const int row = (i >> 3) * H + jg * 8 + (i & 7);
  const int k0 = 16 * c + 8 * (lane >> 5);
  const float* w = (dir ? whh_b : whh_f) + (size_t)row * H;
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = k0 + j < H ? w[k0 + j] * s : 0.f;
  u32x4_t hi, lo;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (NP == 2) {
      typedef _Float16 h2 __attribute__((ext_vector_type(2)));
      const h2 h = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_pkrtz(x[2 * j], x[2 * j + 1]));
      hi[j] = __builtin_bit_cast(unsigned, h);
      lo[j] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(x[2 * j] - (float)h[0], x[2 * j + 1] - (float)h[1]));
    } else {
      typedef _Float16 h2 __attribute__((ext_vector_type(2)));
      const h2 h = {(_Float16)x[2 * j], (_Float16)x[2 * j + 1]};
      hi[j] = __builtin_bit_cast(unsigned, h);
    }
  }
  u32x4_t* o = wp + ((size_t)((dir * HQ + jg) * NC + c) * NP) * 64 + lane;
  o[0] = hi;
  if (NP == 2) o[64] = lo;
}

struct Lstm16Args {
  const float* xg;
  const u32x4_t* wp;    // lstm_pack16_kernel<NP>
  const float* hdr;     // hdr[0]: accumulator scale
  void* hbuf0;          // [2 dir][NBT][NC][NP][64 lane] x 16 bytes
  void* hbuf1;
  unsigned* flags;      // [2 dir][NBT][H/8] epoch words
  unsigned* err;
  float* out;
  float* gates_save;
  float* c_save;
  int B, T, H, Bpad, bt0;
};

template <int NP>
__global__ __launch_bounds__(256)
void lstm16_persistent_kernel(Lstm16Args a) {
  __shared__ float sRed[3 * 16 * 64];
  __shared__ int sDead;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int HQ = a.H / 8;
  const int NC = (a.H + 15) / 16;
  const int NBT = a.Bpad / 32;
  const int jg = blockIdx.x % HQ;
  const int bt = a.bt0 + blockIdx.x / HQ;
  const int dir = blockIdx.y;
  const int b = bt * 32 + l31;
  if (tid == 0) sDead = 0;

  // W_hh slice: resident for the whole sequence
  const u32x4_t* wq = a.wp + ((size_t)(dir * HQ + jg) * NC * NP) * 64 + lane;
  f16x8 w[kMaxC][NP];
#pragma unroll
  for (int i = 0; i < kMaxC; ++i) {
    const int c = wave + 4 * i;
#pragma unroll
    for (int p = 0; p < NP; ++p) w[i][p] = lstm16_load_w<NP>(wq, c, p, NC);
  }
  const float inv = a.hdr[0];
  const size_t group = (size_t)dir * NBT + bt;
  const unsigned hbytes = (unsigned)((size_t)2 * NBT * NC * NP * 1024);
  __amdgpu_buffer_rsrc_t hrs[2] = {__builtin_amdgcn_make_buffer_rsrc(a.hbuf0, 0, hbytes, 0x00020000),
                                   __builtin_amdgcn_make_buffer_rsrc(a.hbuf1, 0, hbytes, 0x00020000)};
  unsigned* const gflags = a.flags + group * HQ;
  float cprev[4] = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();

#pragma unroll 1
  for (int s = 0; s < a.T; ++s) {
    const int t = dir ? (a.T - 1 - s) : s;
    float xgv[16];
    if (wave == 0) {
      const bool ok = b < a.B;
      const float* xrow = lstm_gate_row(a.xg, (size_t)(ok ? b : 0) * a.T + t, dir, jg, half, a.H);
#pragma unroll
      for (int r = 0; r < 16; ++r) xgv[r] = lstm_gate_at(xrow, r, a.H, ok);
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (s > 0) {
      if (wave == 0 && !sDead) {
        unsigned spins = 0;
        for (;;) {
          bool ok = true;
          for (int j = lane; j < HQ; j += 64)
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
      const unsigned hoff = (unsigned)((group * NC * NP * 64 + lane) * 16);
      f16x8 h[kMaxC][NP];
#pragma unroll
      for (int i = 0; i < kMaxC; ++i) {
        const int c = wave + 4 * i;
#pragma unroll
        for (int p = 0; p < NP; ++p)
          h[i][p] = __builtin_bit_cast(f16x8, c < NC ? __builtin_amdgcn_raw_buffer_load_b128(hrs[s & 1], hoff + (unsigned)(c * NP + p) * 1024u, 0, 16 /* sc1 */)
                                                       : u32x4_t{0u, 0u, 0u, 0u});
      }
#pragma unroll
      for (int i = 0; i < kMaxC; ++i) {
        if (wave + 4 * i < NC) acc = lstm16_mfma_chunk<NP>(w[i], h[i], acc);          // wave-uniform
      }
      // hidden sizes beyond 4*kMaxC*16 = 448: remaining chunks, weights re-read from L2 each step
      for (int c = wave + 4 * kMaxC; c < NC; c += 4) {
        f16x8 wc[NP], hc[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          wc[p] = __builtin_bit_cast(f16x8, wq[(size_t)(c * NP + p) * 64]);
          hc[p] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(hrs[s & 1], hoff + (unsigned)(c * NP + p) * 1024u, 0, 16));
        }
        acc = lstm16_mfma_chunk<NP>(wc, hc, acc);
      }
    }
    if (wave > 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sRed[((wave - 1) * 16 + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int w3 = 0; w3 < 3; ++w3)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += sRed[(w3 * 16 + r) * 64 + lane];
      float hv[4], cnew[4], gact[4][4];
      // (lstm_cell_unit<true>'s arithmetic, written out: as a call beside this kernel's other helpers it moves the NP = 2 stream --
      // profiles/lstm_split.md.  Keep it in step with lstm_common.h.)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float gi = vs_sigmoid_fast(fmaf(acc[0 + u], inv, xgv[0 + u]));
        const float gf = vs_sigmoid_fast(fmaf(acc[4 + u], inv, xgv[4 + u]));
        const float gg = vs_tanh_fast(fmaf(acc[8 + u], inv, xgv[8 + u]));
        const float go = vs_sigmoid_fast(fmaf(acc[12 + u], inv, xgv[12 + u]));
        const float cn = gf * cprev[u] + gi * gg;
        hv[u] = go * vs_tanh_fast(cn);
        cnew[u] = cn;
        cprev[u] = cn;
        gact[0][u] = gi; gact[1][u] = gf; gact[2][u] = gg; gact[3][u] = go;
      }
      // the half-chunk (chunk jg>>1, k-half jg&1) of this lane's column: the lower half-wave stores the hi plane, the upper one the lo plane
      {
        float full[8];
        lstm_gather_half_chunk(full, hv, half);
        const unsigned plane = NP == 2 ? (unsigned)half : 0u;
        const unsigned off = (unsigned)((((group * NC + (jg >> 1)) * NP + plane) * 64 + (jg & 1) * 32 + l31) * 16);
        if (NP == 2 || half == 0)
          __builtin_amdgcn_raw_buffer_store_b128(lstm16_pack_h<NP, false>(full, half), hrs[(s + 1) & 1], off, 0, 16 /* sc1: write-through */);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_store(gflags + jg, (unsigned)(s + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      lstm_store_outputs(a.out, a.c_save, a.gates_save, b, a.B, t, a.T, a.H, dir, jg, half, hv, cnew, gact);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The same recurrence with the hidden vector as its OWN flag (round 5): one agent-scope round trip per step instead
// of two.  The flag protocol above costs, per step and on the critical path: store h (write-through) -> wait for the store to
// drain -> store the flag -> [consumer] see the flag -> load h: two dependent round trips plus the drain.  Here:
//   * FOUR exchange buffers; h_s lives in buffer s % 4.  A slot that has not been written yet holds the SENTINEL 0x7FFF7FFF in
//     every dword -- two 16-bit NaNs, a pattern no finite h (hi or lo plane; bf16 gate gradient in the BPTT) produces;
//   * a consumer wave polls the chunks IT multiplies (sc1 loads, as before) until no dword of them is the sentinel: a dword is
//     written by one store instruction, so it is either old (sentinel) or complete; no flag word, no workgroup barrier in front
//     of the MFMAs;
//   * the producer of a slot re-arms it.  At step s, behind the workgroup barrier of the K reduction -- EVERY wave's poll of h_s has
//     succeeded, so every member of the group has published h_s, i.e. has finished step s - 1 and with it every read of buffer
//     (s - 1) % 4 -- it waits for its older stores (the re-arming store of the previous step among them: a whole step old, the
//     wait is free), stores the sentinel to ITS slot of buffer (s - 1) % 4 = (s + 3) % 4, does the gate arithmetic and stores
//     h_{s+1} into buffer (s + 1) % 4 with nothing behind it.  Why nobody can read stale data: buffer X % 4 is polled for h_X by a
//     consumer that has finished step X - 1, for which it needed this workgroup's h_{X-1}; that was stored at step X - 2 behind the
//     wait that acknowledged the re-arming store of step X - 3, whose target was (X - 3 + 3) % 4 = X % 4.  (Three buffers would do
//     with the acknowledgement exposed inside the step; a re-arm by a wave that has only seen ITS chunks arrive -- the first version
//     -- is a race: a slow member may still be reading the slot.)
// Every spin is bounded and reports through *err (NaN poison + vs_lstm_status as before).  H <= 448 (all chunks register-resident);
// larger hidden sizes take the flag kernel.
// ---------------------------------------------------------------------------------------------

// RAGGED (the eval forward of a padded batch of clips of unequal length, vs_bilstm_fwd_ragged): wave 0's gate arithmetic holds
// h = c = 0 while t >= lengths[b] -- two selects per gate lane, the same schedule and hand-off.  The reverse direction then reaches
// t = lengths[b] - 1 with the zero state of a fresh clip, the forward direction writes zeros past the end.  Selects, not products:
// whatever xg holds in those rows (NaN included) stays out.  !RAGGED is the kernel as it was (lengths unused).
//
// SHARED (several enrolled speakers per mixture, vs_bilstm_fwd_multi): the launch runs N = a.B sequences n = m*K + k, speaker k of
// mixture m.  The d-vector enters the gates only as a row bias that does not depend on t, so the K sequences of a mixture share ONE
// row of gate pre-activations: wave 0 reads xg [N / K][T][8H] (the input GEMM run once, WITHOUT row bias) at mixture n / K -- columns
// of a tile that belong to one mixture read the same row -- and adds the lane's 16 values of sh.rowbias [N][8H], loaded once in front of
// the time loop and held in registers, in fp32 before the gate functions.  lengths (RAGGED) are per mixture: lengths[n / K].  Padding
// columns n >= N behave as b >= B does.  Schedule, hand-off, spins and error word are the kernel's own; !SHARED is the kernel as it
// was (sh unused).
struct LstmSharedIn {
  const float* rowbias;   // [N][8H]: dvec @ W_ih[:, 8F:]^T + b_ih + b_hh of sequence n, both directions
  int K;                  // sequences per shared row of xg
};

//
// CARRY (stream separation chunk by chunk, vs_bilstm_recurrent_carry): the FORWARD direction starts from a caller-given state instead
// of zero and hands its state out at one chosen frame, so the next call continues the same recurrence.  h_0 reaches the workgroups the
// way every later h does: lstm16_seed_kernel, a launch in front of this one on the same stream, writes it into exchange buffer 0 in the
// operand form below (the reverse direction's slots keep the launcher's zeros), and step 0 polls and multiplies like every other step.
// c_0 goes straight into wave 0's registers.  When the forward direction finishes frame t = keep - 1, wave 0 stores h and c of that
// frame in fp32 to state_out [B][2][H] (h, then c), behind the exchange store; the direction runs on to T (its rows t >= keep are the
// forward outputs over the caller's look-ahead frames).  The h handed out is the fp32 value the exchange store rounds, and the seeding
// pass rounds it the same way: two calls over [0, a) and [a, T) give the forward half of one call over [0, T) bit for bit.  Hand-off,
// re-arming, spins and error word are the kernel's own; !CARRY is the kernel as it was (cy unused).
//
// CARRY x SHARED (several enrolled speakers from one live mixture, vs_bilstm_recurrent_carry_shared): both of the above, per column.
// Column n = m*K + k reads xg at mixture n / K and adds its own resident row bias (SHARED); its forward direction starts from
// state_in[n] and hands its state to state_out[n] (CARRY): state, exchange slots and outputs are indexed by the column, only the xg row
// by the mixture.  The seeding pass runs over the N columns.  No other line differs, so what makes the carried state exact -- the h
// handed out is the fp32 value the exchange store rounds, the seed rounds it with lstm16_pack_h<NP, true> -- holds per column.
struct LstmCarry {
  const float* state_in;  // [B][2][H] fp32: h and c of the forward direction in front of frame 0, or NULL: zero (only c is read here)
  float* state_out;       // [B][2][H] fp32: h and c of the forward direction behind frame keep - 1
  int keep;               // 1 <= keep <= T
};

template <int NP, bool RAGGED, bool SHARED = false, bool CARRY = false>
__global__ __launch_bounds__(256)
void lstm16_tagged_kernel(Lstm16Args a, void* hbuf2, void* hbuf3, const int* __restrict__ lengths, LstmSharedIn sh, LstmCarry cy) {
  __shared__ float sRed[2][3 * 16 * 64];      // by step parity: no barrier separates wave 0's reads of step s from the other waves' writes of step s + 1
  __shared__ int sDead;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, half = lane >> 5;
  const int HQ = a.H / 8;
  const int NC = (a.H + 15) / 16;
  const int NBT = a.Bpad / 32;
  const int jg = blockIdx.x % HQ;
  const int bt = a.bt0 + blockIdx.x / HQ;
  const int dir = blockIdx.y;
  const int b = bt * 32 + l31;
  if (tid == 0) sDead = 0;

  const u32x4_t* wq = a.wp + ((size_t)(dir * HQ + jg) * NC * NP) * 64 + lane;
  f16x8 w[kMaxC][NP];
  bool owned[kMaxC];                     // does a producer write this lane's half-chunk?  (the upper half of the last chunk when H % 16 == 8: never)
#pragma unroll
  for (int i = 0; i < kMaxC; ++i) {
    const int c = wave + 4 * i;
    owned[i] = c < NC && 16 * c + 8 * half < a.H;
#pragma unroll
    for (int p = 0; p < NP; ++p) w[i][p] = lstm16_load_w<NP>(wq, c, p, NC);
  }
  const float inv = a.hdr[0];
  const size_t group = (size_t)dir * NBT + bt;
  const unsigned hbytes = (unsigned)((size_t)2 * NBT * NC * NP * 1024);
  __amdgpu_buffer_rsrc_t hrs[4] = {__builtin_amdgcn_make_buffer_rsrc(a.hbuf0, 0, hbytes, 0x00020000),
                                   __builtin_amdgcn_make_buffer_rsrc(a.hbuf1, 0, hbytes, 0x00020000),
                                   __builtin_amdgcn_make_buffer_rsrc(hbuf2, 0, hbytes, 0x00020000),
                                   __builtin_amdgcn_make_buffer_rsrc(hbuf3, 0, hbytes, 0x00020000)};
  // this lane's slot (wave 0 stores it): chunk jg >> 1, k-half jg & 1, plane = lane half (NP == 2) / lower half-wave only (NP == 1)
  const unsigned plane = NP == 2 ? (unsigned)half : 0u;
  const unsigned slot_off = (unsigned)((((group * NC + (jg >> 1)) * NP + plane) * 64 + (jg & 1) * 32 + l31) * 16);
  const bool storer = NP == 2 || half == 0;
  float cprev[4] = {0.f, 0.f, 0.f, 0.f};
  const int xb = SHARED ? b / sh.K : b;          // the row of xg (and of lengths) this column reads
  int len = a.T;
  if (RAGGED) len = b < a.B ? lengths[xb] : 0;
  float rbv[16];                                 // SHARED: this lane's row bias, resident for the whole sequence (wave 0)
  if (SHARED && wave == 0) {
    const bool ok = b < a.B;
    const float* xrow = lstm_gate_row(sh.rowbias, (size_t)(ok ? b : 0), dir, jg, half, a.H);
#pragma unroll
    for (int r = 0; r < 16; ++r) rbv[r] = lstm_gate_at(xrow, r, a.H, ok);
  }
  if (CARRY && wave == 0 && dir == 0 && cy.state_in && b < a.B) {
    const float4 c0 = *reinterpret_cast<const float4*>(cy.state_in + ((size_t)b * 2 + 1) * a.H + jg * 8 + 4 * half);
    cprev[0] = c0.x; cprev[1] = c0.y; cprev[2] = c0.z; cprev[3] = c0.w;
  }
  __syncthreads();

#pragma unroll 1
  for (int s = 0; s < a.T; ++s) {
    const int t = dir ? (a.T - 1 - s) : s;
    const int rb = s & 3, wb = (s + 1) & 3, zb = (s + 3) & 3;            // h_s is read from rb, h_{s+1} goes to wb, zb (= h_{s-1}'s) is re-armed
    float xgv[16];
    if (wave == 0) {
      const bool ok = b < a.B;
      const float* xrow = lstm_gate_row(a.xg, (size_t)(ok ? xb : 0) * a.T + t, dir, jg, half, a.H);
#pragma unroll
      for (int r = 0; r < 16; ++r) xgv[r] = lstm_gate_at(xrow, r, a.H, ok);
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (CARRY || s > 0) {          // CARRY: buffer 0 holds the seeded h_0 (zeros for the reverse direction)
      const unsigned hoff = (unsigned)((group * NC * NP * 64 + lane) * 16);
      f16x8 h[kMaxC][NP];
      unsigned spins = 0;
      for (;;) {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < kMaxC; ++i) {
          const int c = wave + 4 * i;
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            u32x4_t v = c < NC ? __builtin_amdgcn_raw_buffer_load_b128(hrs[rb], hoff + (unsigned)(c * NP + p) * 1024u, 0, 16 /* sc1 */)
                               : u32x4_t{0u, 0u, 0u, 0u};
            if (!owned[i]) v = u32x4_t{0u, 0u, 0u, 0u};
            ok = ok && v[0] != kSentinel && v[1] != kSentinel && v[2] != kSentinel && v[3] != kSentinel;
            h[i][p] = __builtin_bit_cast(f16x8, v);
          }
        }
        if (__all(ok)) break;
        if (++spins > kSpinLimit / 4 || *(volatile int*)&sDead) {      // (a poll round here is 7-13 loads, not one: the same give-up time as the flag kernels')
          lstm_give_up(lane, &sDead, a.err);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
#pragma unroll
      for (int i = 0; i < kMaxC; ++i) {
        if (wave + 4 * i < NC) acc = lstm16_mfma_chunk<NP>(w[i], h[i], acc);          // wave-uniform
      }
    }
    if (wave > 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sRed[s & 1][((wave - 1) * 16 + r) * 64 + lane] = acc[r];
    }
    // wave 1 is the re-arming wave (wave 0's store queue carries h: a sentinel store in front of it would delay it).  Its re-arming
    // store of the previous step is acknowledged HERE, in front of the barrier behind which wave 0 stores this step's h (see the header)
    if (wave == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // every wave's poll has succeeded: the group is done with buffer zb
    if (wave == 1 && s > 0 && storer)
      __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{kSentinel, kSentinel, kSentinel, kSentinel}, hrs[zb], slot_off, 0, 16);
    if (wave == 0) {
#pragma unroll
      for (int w3 = 0; w3 < 3; ++w3)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += sRed[s & 1][(w3 * 16 + r) * 64 + lane];
      if (SHARED) {
#pragma unroll
        for (int r = 0; r < 16; ++r) xgv[r] += rbv[r];
      }
      float hv[4], cnew[4], gact[4][4];
      // (this kernel keeps its own copy of lstm_cell_unit's arithmetic and of lstm_gather_half_chunk + lstm16_pack_h<NP, true>: with
      // either as a call the instruction streams of its instances move -- profiles/lstm_split.md.  Keep them in step with lstm_common.h.)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float gi = vs_sigmoid_fast(fmaf(acc[0 + u], inv, xgv[0 + u]));
        const float gf = vs_sigmoid_fast(fmaf(acc[4 + u], inv, xgv[4 + u]));
        const float gg = vs_tanh_fast(fmaf(acc[8 + u], inv, xgv[8 + u]));
        const float go = vs_sigmoid_fast(fmaf(acc[12 + u], inv, xgv[12 + u]));
        float cn = gf * cprev[u] + gi * gg;
        hv[u] = go * vs_tanh_fast(cn);
        if (RAGGED) {
          cn = t < len ? cn : 0.f;
          hv[u] = t < len ? hv[u] : 0.f;
        }
        cnew[u] = cn;
        cprev[u] = cn;
        gact[0][u] = gi; gact[1][u] = gf; gact[2][u] = gg; gact[3][u] = go;
      }
      {
        float full[8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float o = __shfl_xor(hv[u], 32, 64);
          full[u] = half ? o : hv[u];
          full[4 + u] = half ? hv[u] : o;
        }
        u32x4_t v;
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (NP == 2) {
            const float x0 = full[2 * j] * kHScale, x1 = full[2 * j + 1] * kHScale;
            const h2 hh = __builtin_bit_cast(h2, __builtin_amdgcn_cvt_pkrtz(x0, x1));
            const unsigned lo = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(x0 - (float)hh[0], x1 - (float)hh[1]));
            v[j] = half ? lo : __builtin_bit_cast(unsigned, hh);
          } else {
            const h2 hh = {(_Float16)full[2 * j], (_Float16)full[2 * j + 1]};
            v[j] = __builtin_bit_cast(unsigned, hh);
          }
          v[j] = v[j] == kSentinel ? kUnSentinel : v[j];      // the guard of lstm16_pack_h
        }
        if (storer) __builtin_amdgcn_raw_buffer_store_b128(v, hrs[wb], slot_off, 0, 16 /* sc1: write-through */);
      }
      if (b < a.B) {
        lstm_store_h(a.out, b, t, a.T, a.H, dir, jg, half, hv);
        if (CARRY && dir == 0 && t == cy.keep - 1) {      // the state the next call starts from
          float4* so = reinterpret_cast<float4*>(cy.state_out + (size_t)b * 2 * a.H + jg * 8 + 4 * half);
          so[0] = make_float4(hv[0], hv[1], hv[2], hv[3]);
          so[a.H / 4] = make_float4(cnew[0], cnew[1], cnew[2], cnew[3]);
        }
        lstm_store_tape(a.c_save, a.gates_save, b, t, a.T, a.H, dir, jg, half, cnew, gact);
      }
    }
  }
}

// CARRY's seeding pass: h_0 of the forward direction, state_in [B][2][H] fp32, into exchange buffer 0 in the tagged kernel's operand
// form -- thread (b, jg) converts the 8 values a producer workgroup jg would have stored for batch column b, into the same slot, with
// lstm16_pack_h<NP, true>: its roundings and sentinel guard.  The tagged kernel, which consumes these slots, keeps a written-out copy
// of that packing (see there): bit equality of a carried stream with a whole one holds only while that copy matches lstm16_pack_h
// (tests/test_gpu_stream.py asserts it).  Plain stores: the kernel boundary publishes them.  Everything else in buffer 0 (reverse
// direction, padding columns) keeps the launcher's zeros.
template <int NP>
__global__ void lstm16_seed_kernel(const float* __restrict__ state_in, u32x4_t* __restrict__ hbuf0, int B, int H) {
  const int HQ = H / 8, NC = (H + 15) / 16;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)B * HQ) return;
  const int jg = idx % HQ, b = idx / HQ;
  const int bt = b >> 5, l31 = b & 31;
  const float* hrow = state_in + (size_t)b * 2 * H + jg * 8;
  const float4 lo4 = *reinterpret_cast<const float4*>(hrow), hi4 = *reinterpret_cast<const float4*>(hrow + 4);
  const float full[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
  // group = (dir 0) * NBT + bt; [group][NC][NP][64 lane]
  const size_t slot = (((size_t)bt * NC + (jg >> 1)) * NP) * 64 + (jg & 1) * 32 + l31;
  const u32x4_t vl = lstm16_pack_h<NP, true>(full, 1), vh = lstm16_pack_h<NP, true>(full, 0);
  hbuf0[slot] = vh;
  if (NP == 2) hbuf0[slot + 64] = vl;
}

}  // namespace

// packed recurrent weights: the fp32 fragment form (every arithmetic: the step kernels use it), then room for the f16
// form of the math-selected persistent kernel (two planes), then a 64-float header (accumulator scale, weight scale, |max|)
static size_t lstm_packed_fp32_floats(int H) { return (size_t)2 * (H / 8) * (H / 8) * 256; }
static size_t lstm_packed_f16_floats(int H) { return (size_t)2 * (H / 8) * ((H + 15) / 16) * 2 * 256; }
extern "C" size_t vs_lstm_packed_floats(int H) { return lstm_packed_fp32_floats(H) + lstm_packed_f16_floats(H) + 64; }
// h ping, h pong, flags / c, + a fourth: four regions of 2 * Hp * Bpad floats (Hp = H rounded up to the f16 form's 16-wide K chunk; the
// tagged-data hand-off uses all four as exchange buffers) + 64: the persistent kernels' error word lives in the last 64 floats
// (never touched by the step kernels)
static size_t lstm_state_region(int B, int H) { return (size_t)2 * ((H + 15) / 16 * 16) * (((size_t)B + 31) / 32 * 32); }
extern "C" size_t vs_lstm_state_floats(int B, int H) { return 4 * lstm_state_region(B, H) + 64; }

// math: the dims.math of the call the weights are packed for (VS_MATH_CODE_*); it selects the f16 form written behind
// the fp32 one
int vs_lstm_pack_impl(const float* whh_f, const float* whh_b, float* wp, int H, hipStream_t stream, int math) {
  VS_REQUIRE(H > 0 && H % 8 == 0, "lstm: hidden size %d must be a multiple of 8", H);
  const long long total = (long long)lstm_packed_fp32_floats(H);
  hipLaunchKernelGGL(lstm_pack_whh_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, whh_f, whh_b, wp, H);
  VS_LAUNCH_CHECK();
  if (math == VS_MATH_CODE_FP32) return 0;
  u32x4_t* w16 = reinterpret_cast<u32x4_t*>(wp + lstm_packed_fp32_floats(H));
  float* hdr = wp + lstm_packed_fp32_floats(H) + lstm_packed_f16_floats(H);
  const long long slots = 2LL * (H / 8) * ((H + 15) / 16) * 64;
  if (math == VS_MATH_CODE_BF16) {
    hipLaunchKernelGGL((lstm_pack16_kernel<1>), dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, whh_f, whh_b, w16, hdr, H);
  } else {
    // one power-of-two scale for both directions' W_hh: max|W_hh| * s in [2^9, 2^10)
    unsigned* amax = reinterpret_cast<unsigned*>(hdr + 8);
    VS_CHECK_HIP(hipMemsetAsync(amax, 0, sizeof(unsigned), stream));
    if (int rc = vs_absmax_accum_impl(whh_f, (long long)4 * H * H, amax, stream)) return rc;
    if (int rc = vs_absmax_accum_impl(whh_b, (long long)4 * H * H, amax, stream)) return rc;
    if (int rc = vs_scale_from_absmax_impl(amax, 1, hdr + 1, stream)) return rc;
    hipLaunchKernelGGL((lstm_pack16_kernel<2>), dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, whh_f, whh_b, w16, hdr, H);
  }
  VS_LAUNCH_CHECK();
  return 0;
}

// which recurrence runs: 0 = persistent when its grid is resident (default), 1 = one launch per step (fp32 MFMA),
// 2 = persistent (error if it cannot be), 3 = persistent with the fp32 MFMA products whatever dims.math says (A/B of
// the f16 / bf16 products), 4 = persistent with the flag protocol of rounds 2-4 where the default is the tagged-data hand-off
// (lstm16_tagged_kernel: the f16 forward recurrence; the BPTT has the flag protocol alone).  Test / A-B switch, process-global;
// lstm_bwd.hip reads it through vs_lstm_kernel_mode.
static int g_lstm_kernel = 0;
extern "C" int vs_set_lstm_kernel(int mode) {
  VS_REQUIRE(mode >= 0 && mode <= 4, "vs_set_lstm_kernel: mode %d", mode);
  g_lstm_kernel = mode;
  return 0;
}
int vs_lstm_kernel_mode() { return g_lstm_kernel; }

// What the carry form can be refused for without looking at the device: checked by both C entries before anything else
int vs_lstm_carry_check(int math, int H, int T, int keep, const float* state_out, const char* what) {
  VS_REQUIRE(state_out != nullptr, "%s: state_out is NULL", what);
  VS_REQUIRE(keep >= 1 && keep <= T, "%s: keep=%d outside 1 <= keep <= T = %d", what, keep, T);
  VS_REQUIRE(math == VS_MATH_CODE_F16X3 || math == VS_MATH_CODE_BF16,
             "%s: the carried state is served by VS_MATH_F16X3 and VS_MATH_BF16; VS_MATH_FP32 has no carry recurrence", what);
  VS_REQUIRE(H <= 64 * kMaxC, "%s: H=%d: the carried state is served by the tagged recurrence (H <= %d); the flag kernel starts from a zero state",
             what, H, 64 * kMaxC);
  VS_REQUIRE(g_lstm_kernel == 0 || g_lstm_kernel == 2,
             "%s: vs_set_lstm_kernel(%d) selects a recurrence that starts from a zero state; the carried state needs mode 0 or 2", what, g_lstm_kernel);
  return 0;
}

// the raw carry recurrence beside vs_bilstm_recurrent_math (see the header)
extern "C" int vs_bilstm_recurrent_carry(const float* xg, const float* packed_whh, float* state, float* out, const float* state_in,
                                         float* state_out, int keep, int B, int T, int H, int math, void* stream) {
  VS_REQUIRE(math == VS_MATH_CODE_FP32 || math == VS_MATH_CODE_F16X3 || math == VS_MATH_CODE_BF16, "bilstm_recurrent_carry: unknown math %d", math);
  VS_REQUIRE(B > 0 && T > 0 && H > 0 && H % 8 == 0, "bilstm_recurrent_carry: bad shape B=%d T=%d H=%d (H must be a multiple of 8)", B, T, H);
  if (int rc = vs_lstm_carry_check(math, H, T, keep, state_out, "bilstm_recurrent_carry")) return rc;
  VS_REQUIRE(xg && packed_whh && state && out, "bilstm_recurrent_carry: NULL argument");
  const VsLstmCarry carry{state_in, state_out, keep};
  return vs_bilstm_recurrent_impl(xg, packed_whh, state, out, nullptr, nullptr, B, T, H, (hipStream_t)stream, math, nullptr, nullptr, 1, &carry);
}

// the raw carry x shared-input recurrence: N = M * K sequences, sequence n reads row n / K of xg (see the header)
extern "C" int vs_bilstm_recurrent_carry_shared(const float* xg, const float* rowbias, int K, const float* packed_whh, float* state, float* out,
                                                const float* state_in, float* state_out, int keep, int N, int T, int H, int math, void* stream) {
  const char* what = "bilstm_recurrent_carry_shared";
  VS_REQUIRE(math == VS_MATH_CODE_FP32 || math == VS_MATH_CODE_F16X3 || math == VS_MATH_CODE_BF16, "%s: unknown math %d", what, math);
  VS_REQUIRE(N > 0 && T > 0 && H > 0 && H % 8 == 0, "%s: bad shape N=%d T=%d H=%d (H must be a multiple of 8)", what, N, T, H);
  VS_REQUIRE(K >= 1, "%s: K=%d speakers per mixture (K >= 1)", what, K);
  VS_REQUIRE(N % K == 0, "%s: N=%d sequences are not a multiple of K=%d", what, N, K);
  if (int rc = vs_lstm_carry_check(math, H, T, keep, state_out, what)) return rc;
  VS_REQUIRE(xg && rowbias && packed_whh && state && out, "%s: NULL argument", what);
  const VsLstmCarry carry{state_in, state_out, keep};
  return vs_bilstm_recurrent_impl(xg, packed_whh, state, out, nullptr, nullptr, N, T, H, (hipStream_t)stream, math, nullptr, rowbias, K, &carry);
}

namespace {
// A persistent launch whose spin gave up (a workgroup was not resident: the error word is 1) has produced garbage.
// The word is only read by callers that ask (vs_lstm_status), so the result itself is made unusable: NaN in the first
// 64 outputs -> NaN mask / NaN gradients -> the training loop's loss guard (train.py:112-114) and every isfinite check
// fire instead of training on wrong numbers.
__global__ void lstm_poison_kernel(const unsigned* __restrict__ err, float* __restrict__ out, int n) {
  if (*err == 0u) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = __uint_as_float(0x7fc00000u);
}

// The twelve instances of lstm16_tagged_kernel.  The carry form takes a row bias (CARRY x SHARED) but no lengths: no CARRY x RAGGED
// instance.
const void* lstm16_tagged_instance(int np, bool ragged, bool shared, bool carry) {
#define VS_TAGGED(...) reinterpret_cast<const void*>(&lstm16_tagged_kernel<__VA_ARGS__>)
  static const void* const plain[2][2][2] = {{{VS_TAGGED(1, false, false), VS_TAGGED(1, false, true)}, {VS_TAGGED(1, true, false), VS_TAGGED(1, true, true)}},
                                             {{VS_TAGGED(2, false, false), VS_TAGGED(2, false, true)}, {VS_TAGGED(2, true, false), VS_TAGGED(2, true, true)}}};
  static const void* const carried[2][2] = {{VS_TAGGED(1, false, false, true), VS_TAGGED(1, false, true, true)},
                                            {VS_TAGGED(2, false, false, true), VS_TAGGED(2, false, true, true)}};
#undef VS_TAGGED
  return carry ? carried[np - 1][shared] : plain[np - 1][ragged][shared];
}

// What the tagged persistent recurrence in eval mode alone serves, and how its two refusals read: anything else refuses such a call,
// nothing computes it some other way
struct LstmTaggedOnly { const char *name, *claim, *also, *tail; };
const LstmTaggedOnly kLengthsOnly{"per-item lengths", "per-item lengths need the tagged persistent recurrence in eval mode", "", "do not take them"};
const LstmTaggedOnly kSharedOnly{"shared-input recurrence",
                                 "the shared-input recurrence (several speakers per mixture) is the tagged persistent recurrence in eval mode", "",
                                 "do not offer it"};
const LstmTaggedOnly kCarryOnly{"carried state", "the carried state is served by the tagged persistent recurrence in eval mode alone",
                                ", no lengths", "start from a zero state"};
int lstm_refuse_not_tagged(const LstmTaggedOnly& f, int HQ, int cus) {
  vs_set_error("lstm: %s (dims.math F16X3 or BF16, H <= %d, 2*H/8 = %d workgroups <= %d CUs, vs_set_lstm_kernel 0 or 2%s); VS_MATH_FP32, the flag "
               "kernel and the per-step kernels %s", f.claim, 64 * kMaxC, 2 * HQ, cus, f.also, f.tail);
  return -1;
}
int lstm_refuse_not_resident(const LstmTaggedOnly& f, hipError_t e) {
  vs_set_error("lstm: %s: the persistent recurrence could not be launched resident (%s) and the per-step kernels %s", f.name, hipGetErrorString(e), f.tail);
  return -1;
}
}  // namespace

int vs_lstm_poison_impl(const unsigned* err, float* out, long long n, hipStream_t stream) {
  hipLaunchKernelGGL(lstm_poison_kernel, dim3(1), dim3(64), 0, stream, err, out, (int)(n < 64 ? n : 64));
  VS_LAUNCH_CHECK();
  return 0;
}

// state: four regions of lstm_state_region floats + 64 (vs_lstm_state_floats), zeroed here (zero initial state).  Step kernels: h ping, h pong,
// c.  Flag kernels: h ping, h pong (fragment order), the flag words.  Tagged kernel: four exchange buffers.  The error word is the first of
// the 64 trailing words.
// rowbias != NULL: the shared-input form (lstm16_tagged_kernel<.., SHARED>): B sequences n = m*K + k read xg [B / K][T][8H] at mixture
// n / K and add rowbias [B][8H]; lengths, when given, are per mixture [B / K]; out [B][T][2H]
// carry != NULL: the carry form (lstm16_tagged_kernel<.., CARRY>): the forward direction starts from carry->state_in and hands its
// state behind frame carry->keep - 1 to carry->state_out.  With rowbias too (lstm16_tagged_kernel<.., SHARED, CARRY>) the state is per
// sequence, [B][2][H] with B = the B * K of the caller; with lengths it is refused
int vs_bilstm_recurrent_impl(const float* xg, const float* wp, float* state, float* out, float* gates_save, float* c_save,
                             int B, int T, int H, hipStream_t stream, int math, const int* lengths, const float* rowbias, int K,
                             const VsLstmCarry* carry) {
  VS_REQUIRE(B > 0 && T > 0 && H > 0 && H % 8 == 0, "lstm: bad shape B=%d T=%d H=%d (H must be a multiple of 8)", B, T, H);
  if (carry) { if (int rc = vs_lstm_carry_check(math, H, T, carry->keep, carry->state_out, "lstm")) return rc; }
  VS_REQUIRE(rowbias ? (K >= 1 && B % K == 0) : K == 1, "lstm: %d sequences do not share rows of xg in groups of K=%d", B, K);
  const int Bpad = (B + 31) / 32 * 32;
  const size_t per = lstm_state_region(B, H);
  if (g_lstm_kernel == 3) math = VS_MATH_CODE_FP32;
  VS_CHECK_HIP(hipMemsetAsync(state, 0, vs_lstm_state_floats(B, H) * sizeof(float), stream));
  float* hbuf[2] = {state, state + per};
  const int HQ = H / 8, NBT = Bpad / 32;
  int bt_per_launch = 0, cus = 0;
  if (int rc = lstm_tiles_per_launch(2 * HQ, &bt_per_launch, &cus)) return rc;
  const bool persistent = g_lstm_kernel != 1 && bt_per_launch >= 1;
  VS_REQUIRE(g_lstm_kernel != 2 || persistent, "lstm: persistent recurrence needs 2*H/8 = %d workgroups <= %d CUs", 2 * HQ, cus);
  // the tagged-data hand-off of the f16 forward recurrence: four exchange buffers (the state's four regions), the last three armed with
  // the sentinel
  const bool tagged = persistent && math != VS_MATH_CODE_FP32 && g_lstm_kernel != 4 && (H + 15) / 16 <= 4 * kMaxC;
  const bool tagged_eval = tagged && !gates_save && !c_save;
  if (lengths && !tagged_eval) return lstm_refuse_not_tagged(kLengthsOnly, HQ, cus);
  if (rowbias && !tagged_eval) return lstm_refuse_not_tagged(kSharedOnly, HQ, cus);
  if (carry && !(tagged_eval && !lengths)) return lstm_refuse_not_tagged(kCarryOnly, HQ, cus);
  if (tagged) VS_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(state + per), (int)kSentinel, 3 * per, stream));
  if (carry && carry->state_in) {          // h_0 of the forward direction into exchange buffer 0 (zeroed above), in the kernel's operand form
    const long long n = (long long)B * HQ;
    if (math == VS_MATH_CODE_BF16)
      hipLaunchKernelGGL((lstm16_seed_kernel<1>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, carry->state_in, reinterpret_cast<u32x4_t*>(state), B, H);
    else
      hipLaunchKernelGGL((lstm16_seed_kernel<2>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, carry->state_in, reinterpret_cast<u32x4_t*>(state), B, H);
    VS_LAUNCH_CHECK();
  }
  if (persistent) {
    unsigned* flags = reinterpret_cast<unsigned*>(state + 2 * per);      // zeroed above
    unsigned* err = reinterpret_cast<unsigned*>(state + 4 * per);         // first of the 64 trailing words
    bool launched = true;
    for (int bt0 = 0; bt0 < NBT; bt0 += bt_per_launch) {
      const int nbt = NBT - bt0 < bt_per_launch ? NBT - bt0 : bt_per_launch;
      hipError_t e;
      if (math == VS_MATH_CODE_FP32) {
        LstmPersistArgs a{xg, wp, hbuf[0], hbuf[1], flags, err, out, gates_save, c_save, B, T, H, Bpad, bt0};
        e = launch_resident(reinterpret_cast<const void*>(&lstm_persistent_kernel), dim3(HQ * nbt, 2), dim3(256), a, stream);
      } else {
        // the f16 form the weights were packed in (vs_lstm_pack_impl with the same math) and its header
        const float* w16 = wp + lstm_packed_fp32_floats(H);
        Lstm16Args a{xg, reinterpret_cast<const u32x4_t*>(w16), w16 + lstm_packed_f16_floats(H), hbuf[0], hbuf[1], flags, err, out,
                     gates_save, c_save, B, T, H, Bpad, bt0};
        const int np = math == VS_MATH_CODE_BF16 ? 1 : 2;
        if (tagged) {
          void* hb2 = state + 2 * per;
          void* hb3 = state + 3 * per;
          LstmSharedIn sh{rowbias, K};
          LstmCarry cy{carry ? carry->state_in : nullptr, carry ? carry->state_out : nullptr, carry ? carry->keep : 0};
          void* params[] = {&a, &hb2, &hb3, &lengths, &sh, &cy};
          e = hipLaunchCooperativeKernel(lstm16_tagged_instance(np, lengths != nullptr, rowbias != nullptr, carry != nullptr), dim3(HQ * nbt, 2),
                                         dim3(256), params, 0, stream);
        } else {
          e = launch_resident(np == 1 ? reinterpret_cast<const void*>(&lstm16_persistent_kernel<1>)
                                      : reinterpret_cast<const void*>(&lstm16_persistent_kernel<2>), dim3(HQ * nbt, 2), dim3(256), a, stream);
        }
      }
      if (e != hipSuccess) {
        (void)hipGetLastError();
        // refused before anything ran (first launch): the step kernels below do the whole job; later: an error
        VS_REQUIRE(bt0 == 0 && g_lstm_kernel != 2, "lstm: persistent recurrence could not be launched resident: %s", hipGetErrorString(e));
        if (lengths) return lstm_refuse_not_resident(kLengthsOnly, e);
        if (rowbias) return lstm_refuse_not_resident(kSharedOnly, e);
        if (carry) return lstm_refuse_not_resident(kCarryOnly, e);
        launched = false;
        break;
      }
    }
    if (launched) return vs_lstm_poison_impl(err, out, (long long)B * T * 2 * H, stream);
  }
  if (tagged) VS_CHECK_HIP(hipMemsetAsync(state, 0, vs_lstm_state_floats(B, H) * sizeof(float), stream));      // refused: un-arm the buffers
  float* c = state + 2 * per;
  dim3 grid(HQ * NBT, 2), block(256);
  for (int s = 0; s < T; ++s) {
    LstmStepArgs a{xg, wp, hbuf[s & 1], hbuf[(s + 1) & 1], c, out, gates_save, c_save, B, T, H, Bpad, s};
    hipLaunchKernelGGL(lstm_step_kernel, grid, block, 0, stream, a);
  }
  VS_LAUNCH_CHECK();
  return 0;
}
