// The arithmetic of fir_fft.hip, one thread's share at a time: a 2048-point complex FFT (Stockham autosort, natural order in and out;
// three radix-8 passes and one radix-4 pass) over a buffer of 2048 complex values, and the two split steps that turn it into the real
// transform of 4096 samples and back.  Everything is written per thread (tid = 0 .. 255) with the barriers left to the caller, so the
// same text runs inside a workgroup (LDS, __syncthreads) and, for a check against a plain fp64 sum, in a host loop over tid.
//
//   pass8_load(buf, T, tid, Ns, v)   v[r] = buf[tid + 256 r] T[tid mod Ns * r * 512 / Ns], then the 8-point DFT of v in registers
//   pass8_store(buf, tid, Ns, v)     buf[(tid - tid mod Ns) 8 + tid mod Ns + r Ns] = v[r]            (every load of the pass comes first)
//   pass4(buf, T, j)                 the last pass (Ns = 512) for butterfly j = 0 .. 511: it reads and writes the same four places
// T[i] = exp(-2 pi i / 4096), i = 0 .. 4095, fp64 values rounded once to fp32 (vs_fir_spectra makes the table).
// Packed spectrum of a real sequence of 4096: S[0] = (X[0], X[2048]) (both real), S[k] = X[k], k = 1 .. 2047.  Both split steps
// leave the factor 2 of the even / odd recombination in place (pack_bin gives 2 X, unpack_bin takes what it is given), and the
// transforms are unscaled: a product of two packed spectra brought back comes out 2^14 times the circular convolution, and the one
// multiplication by 2^-14 at the very end is exact.
// Buffer index i lives at i + (i >> 4): one complex value of padding per sixteen.  By the LDS bank rules (ds_write: bank = dword mod
// 32 per half wave; ds_read_b64: dword mod 64) the stride-8 stores of the first pass then fall on every bank exactly twice per half
// wave, which is the least 32 eight-byte stores can do, and the unit-stride loads cross one pad per half wave (one bank pair twice).
#pragma once

#if defined(__HIPCC__)
#define VS_FFT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define VS_FFT_HD inline
#endif

namespace vs_fft {

constexpr int kM = 2048;                                 // complex points = VS_FIR_FFT_BLOCK
constexpr int kThreads = 256;
constexpr int kBuf = kM + kM / 16;                       // padded buffer length
constexpr int kTable = 4096;

struct cf { float x, y; };

VS_FFT_HD int phys(int i) { return i + (i >> 4); }
VS_FFT_HD cf cadd(cf a, cf b) { return {a.x + b.x, a.y + b.y}; }
VS_FFT_HD cf csub(cf a, cf b) { return {a.x - b.x, a.y - b.y}; }
VS_FFT_HD cf cmul(cf a, cf w) { return {a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
VS_FFT_HD cf mul_mi(cf a) { return {a.y, -a.x}; }         // times -i

// 4-point DFT of b, natural order
VS_FFT_HD void dft4(cf& b0, cf& b1, cf& b2, cf& b3) {
  const cf c0 = cadd(b0, b2), c1 = csub(b0, b2), c2 = cadd(b1, b3), c3 = mul_mi(csub(b1, b3));
  b0 = cadd(c0, c2);
  b1 = cadd(c1, c3);
  b2 = csub(c0, c2);
  b3 = csub(c1, c3);
}

// 8-point DFT of v, natural order: X[2 m] = DFT4(v[n] + v[n + 4])[m], X[2 m + 1] = DFT4((v[n] - v[n + 4]) w8^n)[m]
VS_FFT_HD void dft8(cf* v) {
  const float s = 0.70710678118654752440f;               // sqrt(1/2), rounded once
  cf a0 = cadd(v[0], v[4]), a1 = cadd(v[1], v[5]), a2 = cadd(v[2], v[6]), a3 = cadd(v[3], v[7]);
  cf d0 = csub(v[0], v[4]), d1 = csub(v[1], v[5]), d2 = csub(v[2], v[6]), d3 = csub(v[3], v[7]);
  d1 = {s * (d1.x + d1.y), s * (d1.y - d1.x)};           // w8   = (s, -s)
  d2 = mul_mi(d2);                                       // w8^2 = -i
  d3 = {s * (d3.y - d3.x), -(s * (d3.x + d3.y))};        // w8^3 = (-s, -s)
  dft4(a0, a1, a2, a3);
  dft4(d0, d1, d2, d3);
  v[0] = a0; v[2] = a1; v[4] = a2; v[6] = a3;
  v[1] = d0; v[3] = d1; v[5] = d2; v[7] = d3;
}

VS_FFT_HD void pass8_load(const cf* buf, const cf* T, int tid, int Ns, cf* v) {
  const int k = tid & (Ns - 1), step = k * (512 / Ns);
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = buf[phys(tid + kThreads * r)];
  if (Ns > 1) {
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], T[step * r]);
  }
  dft8(v);
}

VS_FFT_HD void pass8_store(cf* buf, int tid, int Ns, const cf* v) {
  const int k = tid & (Ns - 1), j0 = ((tid - k) << 3) + k;
#pragma unroll
  for (int r = 0; r < 8; ++r) buf[phys(j0 + r * Ns)] = v[r];
}

VS_FFT_HD void pass4(cf* buf, const cf* T, int j) {
  cf b0 = buf[phys(j)], b1 = cmul(buf[phys(j + 512)], T[2 * j]), b2 = cmul(buf[phys(j + 1024)], T[4 * j]),
     b3 = cmul(buf[phys(j + 1536)], T[6 * j]);
  dft4(b0, b1, b2, b3);
  buf[phys(j)] = b0;
  buf[phys(j + 512)] = b1;
  buf[phys(j + 1024)] = b2;
  buf[phys(j + 1536)] = b3;
}

// Z = FFT_2048 of z[m] = (x[2 m], x[2 m + 1]): bin k of the packed spectrum, TWICE its value.  zk = Z[k], zm = Z[(2048 - k) mod 2048].
VS_FFT_HD cf pack_bin(cf zk, cf zm, cf w, int k) {
  if (k == 0) return {2.f * (zk.x + zk.y), 2.f * (zk.x - zk.y)};
  const cf a = {zk.x + zm.x, zk.y - zm.y};               // Z[k] + conj Z[M - k]
  const cf c = {zk.y + zm.y, zm.x - zk.x};               // -i (Z[k] - conj Z[M - k])
  return cadd(a, cmul(c, w));                            // w = T[k]
}

// the other way: yk = S[k], ym = S[2048 - k] of a packed spectrum -> conj of Z'[k] = (Y[k] + conj Y[M - k]) + i conj(w) (Y[k] - conj Y[M - k]),
// what the FORWARD transform takes to give conj(z'): x[2 m] = Re, x[2 m + 1] = -Im of its output
VS_FFT_HD cf unpack_bin(cf yk, cf ym, cf w, int k) {
  if (k == 0) return {yk.x + yk.y, -(yk.x - yk.y)};
  const cf a = {yk.x + ym.x, yk.y - ym.y};
  const cf b = {yk.x - ym.x, yk.y + ym.y};
  const cf d = {b.x * w.x + b.y * w.y, b.y * w.x - b.x * w.y};      // conj(w) b
  return {a.x - d.y, -(a.y + d.x)};
}

}  // namespace vs_fft
