// Shared LDS dense-linear-algebra machinery for the CDNA4 GP kernels:
// blocked in-place Cholesky with look-ahead (8x8 register sub-diagonals)
// and the in-place triangular inverse.  Included by expert_nll.hip and
// laplace.hip.  See expert_nll.hip's header comment for the algorithm.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#ifndef WG
#define WG 512
#endif
#define NB 32

typedef __attribute__((ext_vector_type(4))) float mfma_f32x4_t;

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ inline double block_sum(double v, double* red, int tid) {
  v = wave_sum(v);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    double s = 0;
#pragma unroll
    for (int w = 0; w < WG / 64; ++w) s += red[w];
    red[0] = s;
  }
  __syncthreads();
  double out = red[0];
  __syncthreads();
  return out;
}

// Broadcast of lane `src`'s x to the whole wave, `src` a compile-time
// constant: v_readlane_b32 into an SGPR.  Bitwise what __shfl(x, src, 64)
// returns, without the ds_bpermute round trip through the LDS pipe that
// the other resident waves keep busy.  The wave must be converged.
__device__ inline float bcast_lane(float x, int src) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src));
}

// flat f -> (a, b) with a >= b in a lower triangle (incl. diagonal)
__device__ inline void tri_decode(int f, int& a, int& b) {
  a = (int)((sqrtf(8.f * (float)f + 1.f) - 1.f) * 0.5f);
  while ((a + 1) * (a + 2) / 2 <= f) ++a;
  while (a * (a + 1) / 2 > f) --a;
  b = f - a * (a + 1) / 2;
}

// Vectorized contiguous-contiguous dot: both pointers 16-B aligned at
// index 0 (callers pad their LDS row strides to multiples of 4 floats);
// scalar head to a 4-aligned c, float4 (ds_read_b128) body, scalar tail.
__device__ inline float dotv(const float* p, const float* q, int c0,
                             int c1) {
  float s = 0.f;
  int c = c0;
  for (; c < c1 && (c & 3); ++c) s += p[c] * q[c];
  float4 a4 = {0.f, 0.f, 0.f, 0.f};
  for (; c + 3 < c1; c += 4) {
    const float4 a = *(const float4*)(p + c);
    const float4 b = *(const float4*)(q + c);
    a4.x += a.x * b.x;
    a4.y += a.y * b.y;
    a4.z += a.z * b.z;
    a4.w += a.w * b.w;
  }
  s += (a4.x + a4.y) + (a4.z + a4.w);
  for (; c < c1; ++c) s += p[c] * q[c];
  return s;
}

// dotv(p, q, 0, 8) spelled out as the compiler builds dotv's float4 body
// where the length is a run-time value (the all-thread intra-block
// trailing update this replaces): rounded products added to the four
// partials (v_pk_mul_f32, v_pk_add_f32), not fused; then dotv's fold.
__device__ inline float dot8_unfused(const float* p, const float* q) {
#pragma clang fp contract(off)
  const float4 a0 = *(const float4*)p, b0 = *(const float4*)q;
  const float4 a1 = *(const float4*)(p + 4), b1 = *(const float4*)(q + 4);
  const float m0 = a0.x * b0.x, m1 = a0.y * b0.y;
  const float m2 = a0.z * b0.z, m3 = a0.w * b0.w;
  const float n0 = a1.x * b1.x, n1 = a1.y * b1.y;
  const float n2 = a1.z * b1.z, n3 = a1.w * b1.w;
  const float x = (0.f + m0) + n0, y = (0.f + m1) + n1;
  const float z = (0.f + m2) + n2, w = (0.f + m3) + n3;
  return 0.f + ((x + y) + (z + w));
}

// Vectorized-p x strided-q dot: p 16-B aligned at index 0, q any stride.
__device__ inline float dotm(const float* p, const float* q, int sq,
                             int c0, int c1) {
  float s = 0.f;
  int c = c0;
  for (; c < c1 && (c & 3); ++c) s += p[c] * q[c * sq];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (; c + 3 < c1; c += 4) {
    const float4 a = *(const float4*)(p + c);
    s0 += a.x * q[c * sq];
    s1 += a.y * q[(c + 1) * sq];
    s2 += a.z * q[(c + 2) * sq];
    s3 += a.w * q[(c + 3) * sq];
  }
  s += (s0 + s1) + (s2 + s3);
  for (; c < c1; ++c) s += p[c] * q[c * sq];
  return s;
}

// 4-accumulator strided dot over LDS: sum_{c=c0}^{c1-1} p[c*sp] * q[c*sq]
__device__ inline float dot4(const float* p, int sp, const float* q, int sq,
                             int c0, int c1) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int c = c0;
  for (; c + 3 < c1; c += 4) {
    s0 += p[c * sp] * q[c * sq];
    s1 += p[(c + 1) * sp] * q[(c + 1) * sq];
    s2 += p[(c + 2) * sp] * q[(c + 2) * sq];
    s3 += p[(c + 3) * sp] * q[(c + 3) * sq];
  }
  for (; c < c1; ++c) s0 += p[c * sp] * q[c * sq];
  return (s0 + s1) + (s2 + s3);
}

// Orders one wave's LDS writes before its later LDS reads from other lanes,
// with no workgroup barrier: the DS operations of one wave complete in
// issue order, so all that is needed is that the compiler keeps them on
// their sides of this point (wavefront-scope fence + wave_barrier) and
// that the writes have retired (lgkmcnt).  The wave must be converged.
__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The inverse of one diagonal block (bs <= 32 rows at D, row stride SA)
// assembled from its nq = ceil(bs/8) inverted 8x8 sub-blocks Vq[q][8][8]
// (row-major, zero above the diagonal, identity-padded where the last
// sub-block is short) and the sub-diagonal blocks of L still in D, by
// recursive doubling on v_mfma_f32_16x16x4_f32 (exact f32):
//   level 1: V10 = -V1 (L10 V0) and V32 = -V3 (L32 V2), the two pairs
//            block-diagonal in one 16x16 tile;
//   level 2: V_HL = -V_HH (L_HL V_LL) on the 16x16 halves.
// Each level is two dependent products of 4 MFMAs.  Both operands of a
// product take k = 4 * (lane >> 4) + s at MFMA step s, so the B value a
// lane owes the second product is its own accumulator register s of the
// first (C layout: row 4 * (lane >> 4) + s, column lane & 15): the
// intermediate never passes through LDS.  Level 1's tile carries pair 0 in
// rows 8..15 x columns 0..7 and pair 1 in rows 0..7 x columns 8..15, which
// puts V10 where level 2's V_LL fragment wants it, again in the lane's own
// registers; only V32 comes back from D.  Rows and columns past bs are
// masked to zero and never stored.  One converged wave; the caller orders
// the q-loop's LDS writes before and this function's after.
__device__ inline void assemble_diag_inverse(float* D, const int SA,
                                             const float* Vq, const int bs,
                                             const int nq, const int lane) {
  const int fl = lane & 15, kg = lane >> 4;
  const int fp = fl >> 3, f7 = fl & 7;
  // Every fragment that no product feeds is fetched up front, so that the
  // LDS round trips overlap and the MFMA chain waits once.  A masked
  // element reads index 0 (always inside the buffer) and is then zeroed: a
  // load under a lane condition would be issued, and waited for, in its
  // own branch right before the MFMA that takes it.
  float dg[4];                             // Vq, for the diagonal blocks
#pragma unroll
  for (int u = 0; u < 4; ++u) dg[u] = Vq[lane + 64 * u];
  float a1[4], b1[4], a2[4], a3[4], vd[4], a4[4];
  const int lrow = 16 * fp + 8 + f7;       // row of L_{2p+1,2p}, p = fp
  const bool hrow = 16 + fl < bs;          // row of L_HL (implies nq >= 3)
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int kk = 4 * kg + s, k7 = kk & 7, kp = kk >> 3;
    const bool c1 = kp == fp && lrow < bs;
    const bool c2 = kp == fp && 2 * fp < nq;
    const bool c3 = kp != fp && 2 * kp + 1 < nq;
    const bool c4 = kp == fp && 2 + fp < nq;
    const float x1 = D[c1 ? (size_t)lrow * SA + 16 * fp + k7 : 0];
    const float x2 = Vq[c2 ? (2 * fp) * 64 + k7 * 8 + f7 : 0];
    const float x3 = Vq[c3 ? (2 * kp + 1) * 64 + f7 * 8 + k7 : 0];
    const float x4 = D[hrow ? (size_t)(16 + fl) * SA + kk : 0];
    const float x5 = Vq[c4 ? (2 + fp) * 64 + f7 * 8 + k7 : 0];
    vd[s] = Vq[kp * 64 + k7 * 8 + f7];     // V0 / V1: nq >= 2 here or unused
    a1[s] = c1 ? x1 : 0.f;                 // blockdiag(L10, L32)[fl][kk]
    b1[s] = c2 ? x2 : 0.f;                 // blockdiag(V0, V2)[kk][fl]
    a2[s] = c3 ? x3 : 0.f;                 // V_{2p+1}[f7][k7], p = kp = 1 - fp
    a3[s] = hrow ? x4 : 0.f;               // L_HL[fl][kk]
    a4[s] = c4 ? x5 : 0.f;                 // diagonal blocks of V_HH[fl][kk]
  }
  // the diagonal 8x8 blocks of D <- Vq: L's diagonal blocks have no reader
  // left, and no product reads D there
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = lane >> 3, j = lane & 7; // sub-block u, element (i, j)
    const int gi = u * 8 + i;
    if (gi < bs && j <= i) D[(size_t)gi * SA + u * 8 + j] = dg[u];
  }
  if (nq < 2) return;
  // level 1.  W[kk][j] = (L_{2p+1,2p} V_{2p})[kk & 7][j & 7], p = kk>>3 =
  // j>>3; R[i][j] = sum_kk V_{2p+1}[i & 7][kk & 7] W[kk][j], p = kk>>3 =
  // 1 - i>>3: pair p's product sits in rows of 1 - p, columns of p
  mfma_f32x4_t w = {0.f, 0.f, 0.f, 0.f};
  mfma_f32x4_t r1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s)
    w = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s], b1[s], w, 0, 0, 0);
#pragma unroll
  for (int s = 0; s < 4; ++s)
    r1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[s], w[s], r1, 0, 0, 0);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int row = 4 * kg + s;
    const int gr = 16 * fp + 8 + (row & 7);
    if ((row >> 3) != fp && gr < bs)
      D[(size_t)gr * SA + 16 * fp + f7] = -r1[s];
  }
  if (nq < 3) return;
  // level 2.  W2 = L_HL V_LL; V_LL[kk][j]: its diagonal blocks are V0 and
  // V1, its lower-left block V10 = -r1[s] of this lane
  mfma_f32x4_t w2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int kp = (4 * kg + s) >> 3;
    const float bv = (kp == fp) ? vd[s] : (kp > fp ? -r1[s] : 0.f);
    w2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a3[s], bv, w2, 0, 0, 0);
  }
  // R2 = V_HH W2; V_HH[i][kk]: diagonal blocks V2 and V3 (a4), lower-left
  // block V32, which level 1 has just stored
  wave_lds_sync();
  float a5[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int kk = 4 * kg + s, k7 = kk & 7, kp = kk >> 3;
    const bool c5 = fp > kp && 24 + f7 < bs;
    const float x = D[c5 ? (size_t)(24 + f7) * SA + 16 + k7 : 0];
    a5[s] = c5 ? x : a4[s];
  }
  mfma_f32x4_t r2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s)
    r2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a5[s], w2[s], r2, 0, 0, 0);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int gr = 16 + 4 * kg + s;
    if (gr < bs) D[(size_t)gr * SA + fl] = -r2[s];
  }
}

// In place on the lower triangle of Abuf (k x k, row stride SA):
// K -> L -> V = L^{-1} (lower).  Strict upper of Abuf is never touched.
// log|K| accumulates into misc[0]; *bad set to 1 (indefinite) or 2
// (non-finite pivot) on breakdown.  Tbuf: >= max((k-32)*36, 448) floats
// scratch, 16-B aligned (the diagonal block uses T[0..256)); SA must be a multiple of 4 (vectorized dots).
// All WG threads must call (contains __syncthreads).
__device__ inline void chol_invert_lower(float* Abuf, float* Tbuf,
                                         const int k, const int SA,
                                         const int tid_in, int* bad,
                                         double* misc,
                                         unsigned long long* jclk = nullptr) {
  // jclk (profiling only): accumulated cycles into
  //   [0] phase1  [1] phase2 wall (q-loop + inverse assembly)
  //   [2] wave 0's q-loop span (clocked by thread 0)
  //   [3] waves 1-7's update span (clocked by thread 64)
  //   [4] C2 panel solve  [5] D off-diag trtri
  //   [6] wave 0's inverse-assembly span behind the q-loop (thread 0)
  // tid passes through an empty asm at the top of every block-column
  // iteration: values derived from it are then recomputed per iteration
  // (a few VALU ops) instead of being hoisted and kept live across the
  // whole factorization, which at 6 waves/SIMD meant scratch spills.
  int tid = tid_in;
  const int nblk = (k + NB - 1) / NB;
    // ---- C: blocked in-place Cholesky with look-ahead ----------------
  // Right-looking, restructured so the serial diagonal factorization
  // overlaps the data-parallel trailing update: per column block J,
  //   phase1: apply panel J-1's rank-NB update to COLUMN-BLOCK J only
  //   phase2: wave 0 factors+inverts diag J  ||  waves 1-7 apply panel
  //           J-1's update to the remaining trailing columns
  //   phase3: panel solve for block J (copy + GEMM vs inverted diagonal)
  for (int J = 0; J < nblk; ++J) {
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int jb = J * NB;
    const int bs = min(NB, k - jb);
    float* D = Abuf + (size_t)jb * SA + jb;   // diag block, stride SA
    const int pj = jb - NB;                  // previous panel column offset
    unsigned long long jt0 = 0, jt1 = 0;
    if (jclk && tid == 0) jt0 = wall_clock64();

    if (J > 0) {
      // phase1: update ONLY the diagonal block (rows/cols jb..jb+bs, c<=i)
      // so wave 0 can start factoring immediately; the rest of column-block
      // J and the trailing matrix are updated by waves 1-7 during phase2.
      for (int f = tid; f < bs * bs; f += WG) {
        const int r = f / bs, c = f - r * bs;
        if (c > r) continue;                 // keep the Kb upper cache
        const int i = jb + r, cc = jb + c;
        Abuf[(size_t)i * SA + cc] -=
            dotv(Abuf + (size_t)i * SA + pj,
                 Abuf + (size_t)cc * SA + pj, 0, NB);
      }
      __syncthreads();
    }
    if (jclk && (tid == 0 || tid == 64)) jt1 = wall_clock64();

    // phase2: the q-loop over the 8-column sub-blocks of the diagonal
    // block is wave 0's job alone, with no workgroup barrier inside it:
    // per q the register factor-and-inverse of the 8x8 sub-block, the
    // intra-block panel (one lane per panel row) and the intra-block
    // trailing update (two elements per lane in flight); dependent LDS
    // writes and reads are ordered by wave_lds_sync().  Straight behind
    // the loop wave 0 assembles the block's inverse from the 8x8 inverses
    // (assemble_diag_inverse: 16 MFMAs and one more wave_lds_sync(); that
    // short, it costs less there than behind the barrier, where the
    // column-by-column assembly it replaces had to stay:
    // profiles/PROFILES.md rounds 6 and 7).  Meanwhile waves 1-7 apply
    // panel J-1's update to the rows below this column block in one pass.
    // One __syncthreads() ends phase 2, executed by every wave whatever
    // the pivots do: on a failed pivot wave 0 sets *bad, skips its
    // remaining sub-blocks and the assembly and falls through to it.
    // 8x8 inverses live in T[0..256).
    const int nq = (bs + 7) / 8;
    float* Vq = Tbuf;               // [nq][8][8]
    const int t0r = jb + bs;        // first row below this column block
    const int nrp = k - t0r;
    const int ntri_rest = nrp * (nrp + 1) / 2;
    if (tid < 64) {
      // static priority for the serial diagonal-block wave: its dependent
      // chain is the block's critical path while waves 1-7 stream trailing
      // updates — give it the issue-arbitration edge
      // (MI355X_MICROARCH.md "Two waves per SIMD", item 4)
      __builtin_amdgcn_s_setprio(1);
      int w0ok = 1;                  // wave-uniform: no pivot failed yet
      for (int q = 0; q < nq; ++q) {
        const int qb = q * 8;
        const int sbs = min(8, bs - qb);
        {
          // 8x8 factor and inverse on lanes 0..7, ROW j per lane, cross-lane
          // traffic via bcast_lane (every source lane is a compile-time
          // constant, so no LDS-pipe round trip).  Row-per-lane keeps every
          // runtime-varying access at a STATIC register index: the rank-1
          // scalar is the lane's own row[ss], and the update bounds
          // c in (ss, 7] are compile-time — the earlier column-per-lane
          // version needed l[j] with a runtime lane index, which compiles
          // to an 8-deep v_cmp/cndmask select chain per pivot step.
          // Lanes 8..63 compute duplicates and are masked off every store.
          //
          // One 8-step elimination gives both factors: the multipliers
          // that reduce the sub-block are applied to an identity alongside
          // (inv, row j of it), which leaves inv = Lu^-1 of the unit-lower
          // factor, so V[j][c] = rs_j * inv[c]; and L[j][ss] = row[ss] * rs
          // at step ss.  A step's two updates are independent, so its
          // chain is gather, rsqrt, two multiplies, one FMA.
          const int j = lane & 7;
          float row[8];                 // this lane's row: row[c] = m[j][c]
          float inv[8];                 // row j of the running Lu^-1
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            row[c] = (j < sbs && c < sbs && c <= j)
                         ? D[(size_t)(qb + j) * SA + qb + c]
                         : (c == j ? 1.f : 0.f);
            inv[c] = (c == j) ? 1.f : 0.f;
          }
          bool ok = true, nonfin = false;
          // log|sub-block| via one logf at the end: accumulate the pivot
          // mantissa product and exponent sum (branchless — a per-step
          // `ldet += (double)__logf(piv)` plus isfinite/positivity
          // branches cost ~35 instructions per pivot)
          float mprod = 1.f;
          int expsum = 0;
          float myrs = 1.f;             // this row's pivot 1/sqrt
#pragma unroll
          for (int ss = 0; ss < 8; ++ss) {
            // column ss of the Schur complement, by symmetry also pivot
            // row ss: l[c] = lane c's row[ss]; pinv: row ss of inv, final
            // since step ss-1 (its diagonal is 1)
            float l[8], pinv[8];
#pragma unroll
            for (int c = ss; c < 8; ++c) l[c] = bcast_lane(row[ss], c);
#pragma unroll
            for (int c = 0; c < ss; ++c) pinv[c] = bcast_lane(inv[c], ss);
            const float piv = l[ss];
            if (ss < sbs) {
              const bool fin = isfinite(piv);
              // classify only the FIRST failure (nonfin wins only if it
              // happens while still ok), on piv, before rs is used
              nonfin = nonfin || (ok && !fin);
              ok = ok && fin && (piv > 0.f);
              mprod *= __builtin_amdgcn_frexp_mantf(piv);
              expsum += __builtin_amdgcn_frexp_expf(piv);
            }
            const float rs = rsqrtf(piv);
            if (j == ss) myrs = rs;
            // rows j <= ss get m = 0 (their updates ended at step j)
            const float m = (j > ss) ? row[ss] * (rs * rs) : 0.f;
#pragma unroll
            for (int c = ss + 1; c < 8; ++c)
              row[c] = __builtin_fmaf(-m, l[c], row[c]);
#pragma unroll
            for (int c = 0; c < ss; ++c)
              inv[c] = __builtin_fmaf(-m, pinv[c], inv[c]);
            if (j > ss) inv[ss] = -m;
            row[ss] *= rs;              // L[j][ss]
          }
#pragma unroll
          for (int c = 0; c < 8; ++c) inv[c] *= myrs;   // V[j][c]; 0 for c > j
          if (lane < 8) {
            if (j < sbs) {              // write L back (row j)
#pragma unroll
              for (int c = 0; c < 8; ++c)
                if (c <= j) D[(size_t)(qb + j) * SA + qb + c] = row[c];
            }
            float* vo = Vq + q * 64 + j * 8;     // row j of V, contiguous
            *(float4*)vo = make_float4(inv[0], inv[1], inv[2], inv[3]);
            *(float4*)(vo + 4) = make_float4(inv[4], inv[5], inv[6], inv[7]);
          }
          // ok is the same in every lane (every pivot is a broadcast);
          // the exit decision is taken on lane 0's copy in an SGPR
          w0ok = __builtin_amdgcn_readlane((int)ok, 0);
          if (lane == 0) {
            if (!ok) {
              if (*bad == 0) *bad = nonfin ? 2 : 1;  // sticky: first cause
            } else {
              misc[0] += (double)__logf(mprod)
                         + (double)expsum * 0.6931471805599453;
            }
          }
        }
        if (!w0ok) break;            // wave-uniform; on to the block barrier
        wave_lds_sync();             // L write-back and Vq visible
        // intra-block panel P = A * Vq^T for q: one lane per panel row,
        // the row's 8 inputs in registers, so the row is overwritten by
        // its only reader.  pr > 0 implies a full sub-block (sbs == 8).
        const int p0 = qb + sbs;     // first panel row (local)
        const int pr = bs - p0;      // panel rows (<= 24)
        if (pr > 0) {
          if (lane < pr) {
            float* ap = D + (size_t)(p0 + lane) * SA + qb;
            const float4 a0 = *(const float4*)ap;
            const float4 a1 = *(const float4*)(ap + 4);
            const float ar[8] = {a0.x, a0.y, a0.z, a0.w,
                                 a1.x, a1.y, a1.z, a1.w};
            const float* vr = Vq + q * 64;
            float o[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
              float sacc = 0.f;
#pragma unroll
              for (int t = 0; t <= c; ++t)
                sacc = __builtin_fmaf(ar[t], vr[c * 8 + t], sacc);
              o[c] = sacc;
            }
            *(float4*)ap = make_float4(o[0], o[1], o[2], o[3]);
            *(float4*)(ap + 4) = make_float4(o[4], o[5], o[6], o[7]);
          }
          wave_lds_sync();           // panel rows visible
          // trailing: lower incl diag of the remaining pr rows of this
          // block, each element less its length-8 dot over the panel
          // columns (dotv's order of summation).  Rows r and pr-1-r
          // share one line of a ceil(pr/2) x (pr+1) grid, which takes
          // one multiply to decode; a lane holds two elements' loads in
          // flight.  For odd pr the middle row is its own partner and
          // the slots past its diagonal are void.
          const int wd = pr + 1, tot = ((pr + 1) >> 1) * wd;
          const float rwd = 1.f / (float)wd;
          for (int f0 = lane; f0 < tot; f0 += 128) {
            float* tp[2];
            const float *pa[2], *pb[2];
            bool on[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const int f = f0 + 64 * u;
              // f < 512 and wd <= 25: (f + 0.5) / wd is at least 0.02
              // from an integer, the float quotient exact after the cast
              const int r = (int)(((float)f + 0.5f) * rwd);
              const int c = f - r * wd;
              const bool lo = c <= r;
              on[u] = f < tot && (lo || pr - 1 - r != r);
              const int a = on[u] ? (lo ? r : pr - 1 - r) : 0;
              const int b = on[u] ? (lo ? c : c - r - 1) : 0;
              tp[u] = D + (size_t)(p0 + a) * SA + p0 + b;
              pa[u] = D + (size_t)(p0 + a) * SA + qb;
              pb[u] = D + (size_t)(p0 + b) * SA + qb;
            }
            // both dots before either store: the loads issue together
            const float s0 = dot8_unfused(pa[0], pb[0]);
            const float s1 = dot8_unfused(pa[1], pb[1]);
            if (on[0]) *tp[0] -= s0;
            if (on[1]) *tp[1] -= s1;
          }
          wave_lds_sync();           // next sub-block's inputs visible
        }
      }
      unsigned long long jt2 = 0;
      if (jclk && tid == 0) {
        jt2 = wall_clock64();
        jclk[2] += jt2 - jt1;
      }
      // the 32x32 inverse straight behind the q-loop, whose last
      // wave_lds_sync() has made L and Vq visible to this wave
      if (w0ok) assemble_diag_inverse(D, SA, Vq, bs, nq, lane);
      __builtin_amdgcn_s_setprio(0);
      if (jclk && tid == 0) jclk[6] += wall_clock64() - jt2;
    } else if (J > 0) {
      // waves 1-7, one pass: previous panel's update to (a) the panel
      // rows of column-block J and (b) the remaining trailing triangle
      for (int f = tid - 64; f < nrp * bs; f += WG - 64) {
        const int r = f / bs, c = f - r * bs;
        const int i = t0r + r, cc = jb + c;
        Abuf[(size_t)i * SA + cc] -=
            dotv(Abuf + (size_t)i * SA + pj,
                 Abuf + (size_t)cc * SA + pj, 0, NB);
      }
      for (int f = tid - 64; f < ntri_rest; f += WG - 64) {
        int a, b;
        tri_decode(f, a, b);
        const int i = t0r + a, c = t0r + b;
        Abuf[(size_t)i * SA + c] -=
            dotv(Abuf + (size_t)i * SA + pj,
                 Abuf + (size_t)c * SA + pj, 0, NB);
      }
      if (jclk && tid == 64) jclk[3] += wall_clock64() - jt1;
    }
    // phase 2's one barrier: every wave arrives here whatever happened
    // above (no workgroup barrier and no return inside either branch); it
    // publishes the assembled inverse of the diagonal block
    __syncthreads();
    if (jclk && tid == 0) {
      const unsigned long long t2 = wall_clock64();
      jclk[0] += jt1 - jt0;
      jclk[1] += t2 - jt1;
      jt0 = t2;
    }
    if (*bad) break;

    const int t0 = jb + bs;        // first trailing row
    const int nr = k - t0;         // panel rows
    if (nr > 0) {
      // C2: copy panel below the diag block into T (row r-t0, stride 36)
      for (int f = tid; f < nr * bs; f += WG) {
        int r = f / bs, c = f - r * bs;
        Tbuf[r * 36 + c] = Abuf[(size_t)(t0 + r) * SA + jb + c];
      }
      __syncthreads();
      // C2b (MFMA): panel <- T @ V_JJ^T:
      //   A[t0+r][jb+c] = sum_{t<=c} T[r][t] V_JJ[c][t]
      // B-fragment = V_JJ[c][t] masked to its lower triangle; per-wave
      // register tiles, written straight back to the panel.
      {
        const int w8 = tid >> 6;
        const int fl16 = lane & 15, fkg = lane >> 4;
        const int nti = (nr + 15) / 16, ntj = (bs + 15) / 16;
        for (int t = w8; t < nti * ntj; t += WG / 64) {
          const int ti = t / ntj, tj = t - ti * ntj;
          mfma_f32x4_t a = {0.f, 0.f, 0.f, 0.f};
          const int fr = ti * 16 + fl16;       // T row
          const int fc = tj * 16 + fl16;       // V_JJ row (output col)
          for (int c0 = 0; c0 < bs; c0 += 4) {
            const int tt = c0 + fkg;
            const float av = (fr < nr && tt < bs)
                                 ? Tbuf[fr * 36 + tt] : 0.f;
            const float bv = (fc < bs && tt <= fc)
                                 ? D[(size_t)fc * SA + tt] : 0.f;
            a = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, a, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int gr = ti * 16 + fkg * 4 + r;
            const int gc = tj * 16 + fl16;
            if (gr < nr && gc < bs)
              Abuf[(size_t)(t0 + gr) * SA + jb + gc] = a[r];
          }
        }
      }
      __syncthreads();
    }
    if (jclk && tid == 0) jclk[4] += wall_clock64() - jt0;
  }

  if (*bad) return;
  unsigned long long dt0 = 0;
  if (jclk && tid == 0) dt0 = wall_clock64();
  // ---- D: off-diagonal triangular inverse, in place, J right-to-left
  // V_IJ = -(sum_{K=J+1..I} V_IK L_KJ) L_JJ^-1, both halves as MFMA
  // tiles: the U GEMM masks A-fragments to the lower triangle of the
  // already-inverted trailing V (c <= row) and the second GEMM masks
  // B-fragments to V_JJ's lower triangle (t >= j).
  for (int J = nblk - 2; J >= 0; --J) {
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int jb = J * NB;
    const int bs = NB;                       // J < nblk-1 => full block
    const int t0 = jb + bs;
    const int nr = k - t0;
    const int w8 = tid >> 6;
    const int fl16 = lane & 15, fkg = lane >> 4;
    const int nti = (nr + 15) / 16, ntj = (bs + 15) / 16;
    // U into T: U[r][t] = sum_{c=t0..t0+r} V[t0+r][c] * L[c][jb+t]
    for (int t = w8; t < nti * ntj; t += WG / 64) {
      const int ti = t / ntj, tj = t - ti * ntj;
      mfma_f32x4_t a = {0.f, 0.f, 0.f, 0.f};
      const int fr = t0 + ti * 16 + fl16;        // V row (A fragment)
      const int fj = tj * 16 + fl16;             // L column (B fragment)
      for (int c0 = t0; c0 < k; c0 += 4) {
        const int cc = c0 + fkg;
        const float av = (fr < k && cc < k && cc <= fr)
                             ? Abuf[(size_t)fr * SA + cc] : 0.f;
        const float bv = (cc < k && fj < bs)
                             ? Abuf[(size_t)cc * SA + jb + fj] : 0.f;
        a = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, a, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gr = ti * 16 + fkg * 4 + r;
        const int gc = tj * 16 + fl16;
        if (gr < nr && gc < bs) Tbuf[gr * 36 + gc] = a[r];
      }
    }
    __syncthreads();
    // V[t0+r][jb+j] = - sum_{t>=j} U[r][t] * V_JJ[t][j]
    for (int t = w8; t < nti * ntj; t += WG / 64) {
      const int ti = t / ntj, tj = t - ti * ntj;
      mfma_f32x4_t a = {0.f, 0.f, 0.f, 0.f};
      const int fr = ti * 16 + fl16;             // U row (A fragment)
      const int fj = tj * 16 + fl16;             // V_JJ column (B frag)
      for (int c0 = 0; c0 < bs; c0 += 4) {
        const int tt = c0 + fkg;
        const float av = (fr < nr && tt < bs)
                             ? Tbuf[fr * 36 + tt] : 0.f;
        const float bv = (tt < bs && fj < bs && tt >= fj)
                             ? Abuf[(size_t)(jb + tt) * SA + jb + fj]
                             : 0.f;
        a = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, a, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gr = ti * 16 + fkg * 4 + r;
        const int gc = tj * 16 + fl16;
        if (gr < nr && gc < bs)
          Abuf[(size_t)(t0 + gr) * SA + jb + gc] = -a[r];
      }
    }
    __syncthreads();
  }
  if (jclk && tid == 0) jclk[5] += wall_clock64() - dt0;
}

