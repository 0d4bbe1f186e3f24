// Order-16 fused subband update, one wavefront per frequency bin; every dense 16x16x16 contraction is on the
// matrix cores.
//
//   stage 0  R_B, R_D = X^H X, r = X_B^H d        MFMA 16x16x4 (f64 or f32), slab read once, coalesced
//   stage 1  Cholesky of R_D + reg I TOGETHER WITH W = L^-1 (elimination applied to [B | I]); rows of B and W
//            live in registers, one column / one row is broadcast through LDS per step      apvast.py:22-27
//   stage 2  C = W R_B W^H                         two MFMA products (f64: (W R_B)^T, then C's real tile from registers)   apvast.py:28-29
//   stage 3  eigenvectors of C                                                                apvast.py:30
//            float64: a float32 pre-solve -- Householder tridiagonal, Sturm multisection and inverse iteration
//            (tridiag_presolve16) -- then one or two refinement steps of its eigenvector matrix on the f64 MFMA
//            (four complex products each, Ogita & Aishima 2018); a wave whose spectrum has a gap too narrow for that
//            orthonormalises exactly, re-forms C on the MFMA and runs register-resident double sweeps (XOR pairing schedule)
//            float32: the one-sided Jacobi is the solve
//   stage 4  sort                                                                            apvast.py:32-35
//   stage 5  g = W r                               (X = W^H Q, apvast.py:31, only for a caller that asks for U)
//   stage 6  w_V = W^H sum_{i<V} (q_i^H g)/(lam_i+mu) q_i   = sum_{i<V} (x_i^H r)/(lam_i+mu) x_i      apvast.py:406-414
//
// Against a textbook arrangement this removes 48 of the 64 sequential substitution steps (the two forward
// substitutions and the backward one become three MFMA products) and needs two LDS matrices (10 KiB per wave).
#include "apv_internal.h"

#include <cstdlib>

#include "gevd16_common.h"

namespace {

// ---- float32 pre-solve of the float64 kernel: Householder tridiagonal, Sturm multisection, inverse iteration ----------------
// (NumPy model with the same steps and counts: tools/probes/tridiag_presolve_model.py)
__device__ __forceinline__ float tp_lane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
// v of lane `src` (ds_bpermute: a crossbar trip, no LDS storage and no barrier)
__device__ __forceinline__ float tp_from(float v, int src) { return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v))); }
// v of lane (lane & ~3) + j of the quad (quad_perm [j,j,j,j]; j a constant once the reflector loop is unrolled)
__device__ __forceinline__ float tp_quad_bcast(float v, int j) {
    const int x = __float_as_int(v);
    return __int_as_float(j == 0 ? __builtin_amdgcn_mov_dpp(x, 0x00, 0xf, 0xf, false) : j == 1 ? __builtin_amdgcn_mov_dpp(x, 0x55, 0xf, 0xf, false)
                          : j == 2 ? __builtin_amdgcn_mov_dpp(x, 0xAA, 0xf, 0xf, false) : __builtin_amdgcn_mov_dpp(x, 0xFF, 0xf, 0xf, false));
}
// One stage of a cross-lane sum as ONE v_add_f32_dpp (update_dpp with a zero `old` and bound_ctrl is the form the DPP combiner folds
// into the add; a v_mov_b32_dpp and an add otherwise).  The empty asm statement pins the order and keeps the vectoriser from pairing
// two chains into a v_pk_add_f32 fed by moves: chains called alternately fill each other's DPP wait states.
template <int CTRL> __device__ __forceinline__ void tp_dpp_add(float& v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
    asm volatile("" : "+v"(v));
}
// sum over the four lanes of a quad (one matrix row), in all of them: quad_perm [1,0,3,2] and [2,3,0,1]
__device__ __forceinline__ float tp_sum_quad(float v) { tp_dpp_add<0xB1>(v); tp_dpp_add<0x4E>(v); return v; }
// sum over the sixteen quads of a value every lane of a quad holds, as a wave-uniform scalar: row_ror 8 and 4 inside a 16-lane
// row, then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3 (the rows outside the mask keep their value:
// destination and source are one register), which leaves the total in lane 63, and one v_readlane_b32.  Both users want the
// value in a scalar register; delivering it to all 64 lanes took two v_permlane swaps with a move and an add each.  The DPP
// combiner does not produce the masked form, so the two adds are assembly, and they carry their own two wait states in front
// of a DPP read of a VALU result.
__device__ __forceinline__ float tp_sum_quads(float v) {
    tp_dpp_add<0x128>(v);                                                                          // row_ror:8
    tp_dpp_add<0x124>(v);                                                                          // row_ror:4
    asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf" : "+v"(v));
    return tp_lane(v, 63);
}
// Complex multiply-accumulate on (re, im) pairs with the swap and the sign of the imaginary unit as operand modifiers of
// v_pk_fma_f32: acc += (i z) s.y = (-z.y s.y, z.x s.y).  With acc += z s.x (plain source, the compiler folds the broadcast and
// a negation of z into op_sel_hi and neg_lo / neg_hi) it makes acc += z s; with acc -= z s.x it makes acc -= z conj(s).  The
// compiler does not fold the swap-and-negate form, hence the assembly.  Callers end an accumulation that feeds a DPP add with a
// compiler-emitted instruction: the hazard recogniser does not count wait states after an asm statement.
__device__ __forceinline__ void tp_fma_iy(f2v& acc, f2v z, f2v s) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]" : "+v"(acc) : "v"(z), "v"(s));
}
// v in the lanes of a compile-time lane mask, zero in the others: one v_cndmask_b32 on a mask in a scalar pair.  The rows a
// reflector acts on are known once the reflector loop is unrolled; as a test of the row index every mask cost a v_cmp, and the
// fifteen of them, scheduled early, filled the scalar file until masks were spilled into lanes of a VGPR.  The mask is `bits`
// shifted up by `sh` lanes, formed by s_lshl_b64 from an inline constant: handed over as a 64-bit constant it came out as an
// s_mov_b64 with a 32-bit literal, which is right only for the masks whose upper half is the literal's extension.
__device__ __forceinline__ unsigned long long tp_lanes(long long bits, int sh) {
    unsigned long long m;
    if (bits == -1) asm("s_lshl_b64 %0, -1, %1" : "=s"(m) : "s"(sh) : "scc");
    else asm("s_lshl_b64 %0, 15, %1" : "=s"(m) : "s"(sh) : "scc");
    return m;
}
__device__ __forceinline__ float tp_keep(float v, unsigned long long mask) {
    float r;
    asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(v), "s"(mask));
    return r;
}
__device__ __forceinline__ f2v tp_mul_iy(f2v z, f2v s) {                                           // (i z) s.y
    f2v r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1] neg_lo:[1,0]" : "=v"(r) : "v"(z), "v"(s));
    return r;
}
// The wide multisection step's votes: nb_m = the number of lanes whose Sturm count is <= m (one v_cmp into a scalar pair and a
// scalar population count) goes into lane m of nbv, m = M .. 15 (v_writelane_b32 with the lane as an immediate; the compiler has
// no builtin for it)
template <int M> __device__ __forceinline__ void tp_vote(int cnt, int& nbv) {
    const int nb = __builtin_popcountll(__builtin_amdgcn_ballot_w64(cnt <= M));
    asm("v_writelane_b32 %0, %1, %2" : "+v"(nbv) : "s"(nb), "n"(M));
    if constexpr (M + 1 < 16) tp_vote<M + 1>(cnt, nbv);
}

// Multisection: the interval [-1e-3, 1.001] ||C|| (width 1.002 ||C||) shrinks 65x in the wave-wide first step, where all
// sixteen quads still search the same interval and the 64 lanes evaluate 64 distinct points, and 5x in each of the kTpQuadSteps
// quad steps that follow (four points per eigenvalue): 1 + kTpQuadSteps Sturm evaluations per lane.  The refinement certifies the
// result whatever the pre-solve delivers, so the multisection stops where the refinement's own guards stop gaining
// (tools/probes/tridiag_presolve_model.py on the bench bins; DESIGN 4.1 has the table: six quad steps keep the share of bins
// inside the one-step guard, five lose 0.2 %).
constexpr int kTpQuadSteps = 6;
constexpr float tp_pow5_inv(int n) { return n == 0 ? 1.f : 0.2f * tp_pow5_inv(n - 1); }
// width of the final interval in units of ||C||: 1.002 / (65 * 5^kTpQuadSteps) = 9.9e-7
constexpr float kTpFinal = 1.002f / 65.f * tp_pow5_inv(kTpQuadSteps);
// Largest error of the eigenvalue a quad reports, in units of ||C||.  The four lanes of a quad shift by the points 1/8, 3/8, 5/8
// and 7/8 of the final interval and the best one is the quad's eigenvalue, so an eigenvalue inside the interval is at most an
// eighth of the interval from the nearest shift: 0.125 kTpFinal = 1.2e-7.  To that comes the float32 floor of the Sturm count
// and of the interval's re-formed ends, taken as 1e-6: the model's largest error over 32 768 bench bins is 7.2e-7 where the
// interval no longer matters (with this scheme: 6.2e-7 over 32 768, 6.4e-7 with 1-ulp noise on the pivots' reciprocals).
constexpr float kTpLamErr = 0.125f * kTpFinal + 1e-6f;
// Two eigenvalues whose TRUE gap is below 1e-5 ||C|| must not be trusted (see the gate).  Each measured eigenvalue is off by at most
// kTpLamErr, so a true gap g reads as at most g + 2 kTpLamErr: the measured gap has to exceed 1e-5 + 2 kTpLamErr = 1.22e-5 before
// the pair counts as apart.
constexpr float kTpApart = 1e-5f + 2.f * kTpLamErr;
constexpr int LDQ = 17, LDX = 17;       // row strides of the float Q and X in the pre-solve's LDS scratch
constexpr int LDG = 17;                 // row stride, in reals, of stage 2's real tile G (odd: rows and columns both spread over the banks)

// In: C (float64, LDS row stride LD) scaled by 2^sexp, normS2 = ||2^sexp C||_F^2.  Scratch: fQ (16 x LDQ complex), fX (16 x LDX
// real).  Out: V32 (eigenvectors of C in float32, the f32 MFMA accumulator layout: v[t] is element
// (mfma_row<float>(lane, t), lane & 15)), and whether its spectrum is fit for the refinement (finite, spread < 1e3, no two
// eigenvalues closer than 1e-5 ||C||).  The eigenvalues are good to kTpLamErr ||C|| only: the multisection stops where two
// inverse-iteration steps and the refinement's guards (|Z| <= 3e-5 for one step, 1e-2 for two) no longer gain from a finer
// shift.  Their intervals come out in ascending order, quad i holding eigenvalue i, which the gate at the end relies on.
// `stamp` (diagnostic instantiation): slots 4 after the reduction, 13 after the multisection, 14 after the inverse iteration, 5 at the end.
template <typename TS, typename ST = NoStamp>
__device__ __forceinline__ bool tridiag_presolve16(const Cx<TS>* sA, int sexp, float normS2, Cx<float>* fQ, float* fX,
                                                   int lane, Cx<float> v32[4], ST stamp = ST()) {
    using CF = Cx<float>;
    const int i = lane >> 2, jq = lane & 3;
    // ---- 1. Q^H C Q = T, Hermitian tridiagonal, by Hermitian reflectors H_k = I - gamma u u^H with a REAL gamma: for the column
    // x below the diagonal, alpha = x_0, n^2 = ||x||^2, phi = alpha / |alpha| (1 if alpha = 0), u = x but u_0 = alpha + phi ||x||,
    // gamma = 1 / (n^2 + ||x|| |alpha|) = 2 / ||u||^2.  H_k x = -phi ||x|| e_0: the sub-diagonal of T is complex, and only its
    // modulus ||x|| goes on (e[k], and e2[k] = n^2 for the Sturm recurrence).  The phases are put back at the end:
    // diag(delta)^H T diag(delta) is real with delta_0 = 1, delta_{k+1} = -delta_k phi_k, and Q's column m is scaled by delta_m.
    // u needs no scaling (rows beyond k+1 take the raw column entry) and a column with nothing below alpha no special case
    // (u_0 = 2 alpha, H_k a sign flip: the last reflector is compiled as that); a zero column gets gamma = 0.
    // Lane (i, jq) holds A[i][jq + 4 t] and Q[i][jq + 4 t].  The rank-2 updates run on whole rows: rows and columns <= k only
    // collect garbage that is never read again (u is zero there).
    // delta_m is the same in every lane and wanted once, at the end, by the lanes of column m: it waits in LDS (the first 32 floats
    // of fX, free until the inverse iteration; one wave, whose LDS accesses execute in order), not in eight registers per lane
    f2v a[4], q[4];
    f2v* const sdel = reinterpret_cast<f2v*>(fX);
    sdel[0] = (f2v){1.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const Cx<TS> c = sA[i * LD + jq + 4 * t];
        a[t] = (f2v){scale_to_f32(c.x, sexp), scale_to_f32(c.y, sexp)};
        q[t] = (f2v){(jq + 4 * t == i) ? 1.f : 0.f, 0.f};
    }
    // u and w are formed once per row (quad i: A[i][k] by a quad broadcast) and every lane fetches the entries of its own columns
    // jq + 4 t from quad jq + 4 t; ||x||^2 and u^H A u are summed over the quads on the VALU into a scalar register.
    // The fetch goes through LDS (the scratch behind fX, free throughout): the quads write their element, element i to place
    // 4 (i & 3) + (i >> 2), so that the elements jq + 4 t of a lane's slots lie side by side: one ds_write_b64 and one or two
    // ds_read_b128 where the crossbar took up to eight ds_bpermute.  It is a move, so every bit of the result stays, and the
    // kernel is 2 % faster for it (measured; DESIGN 4.1, "The reduction's crossbar trips through LDS", also has what is only
    // inferred about why: the 16 waves of a CU share one LDS and crossbar).  One wave, whose LDS accesses execute in order: no barrier,
    // and the next vector may take the same place.  The four lanes of a quad hold the same value; each writes a copy of its own
    // (34 dwords apart: sixteen lanes, sixteen bank pairs) and everyone reads copy 0, lane 4 i's, as the crossbar did.
    // the scratch (sB of the caller, N x LD elements of Cx<TS>) holds fQ, fX and the four copies: 3 x 136 + 128 bytes
    constexpr size_t kVecOff = sizeof(CF) * N * LDQ + sizeof(float) * N * LDX;
    static_assert(kVecOff + 3 * 136 + 128 <= sizeof(Cx<TS>) * N * LD, "the pre-solve's scratch no longer fits sB");
    static_assert(kVecOff % 16 == 0, "ds_read_b128 wants 16-byte alignment (the caller declares sB alignas(16))");
    char* const vbuf = reinterpret_cast<char*>(fX + N * LDX);
    f2v* const vput = reinterpret_cast<f2v*>(vbuf + 136 * jq + 8 * (4 * (i & 3) + (i >> 2)));
    const f4v* const vget = reinterpret_cast<const f4v*>(vbuf + 32 * jq);
    auto by_column = [&](f2v v, f2v (&c)[4], int first) {                  // slots first .. 3 (first is a constant once unrolled)
        *vput = v;
        if (first < 2) {
            const f4v lo = vget[0];
            c[0] = (f2v){lo.x, lo.y}; c[1] = (f2v){lo.z, lo.w};
        }
        const f4v hi = vget[1];
        c[2] = (f2v){hi.x, hi.y}; c[3] = (f2v){hi.z, hi.w};
    };
    float e[N - 1], e2[N - 1];                                             // |sub-diagonal| and its square (wave-uniform)
    float dlr = 1.f, dli = 0.f;                                            // delta_k (the same in every lane)
#pragma unroll
    for (int k = 0; k < N - 2; ++k) {
        const int t0 = (k + 1) >> 2;                                       // slots 0 .. t0-1 lie in columns <= k: u is zero there
        const int k1 = k + 1, tk = k >> 2, jk = k & 3;
        // A[i][k] to every lane of quad i
        const float akx = tp_quad_bcast(a[tk].x, jk), aky = tp_quad_bcast(a[tk].y, jk);
        // n^2 and alpha from the very column entries u is made of (row k is their conjugate only up to the rounding of the
        // updates, and 1e-7 ||A|| is 1e-5 of a small column: H_k would be that far from unitary).  Every quad adds 1e-31 (the
        // addend of an FMA): e2 is never zero (0 * inf in the Sturm recurrence would be NaN), at no instruction.
        // the column below the diagonal: zero in the rows <= k (quads 0 .. k)
        const unsigned long long low = tp_lanes(-1, 4 * k1);
        const float bx = tp_keep(akx, low), by = tp_keep(aky, low);
        const float n2 = tp_sum_quads(fmaf(bx, bx, fmaf(by, by, 1e-31f)));
        const float alr = tp_lane(akx, 4 * k1), ali = tp_lane(aky, 4 * k1);
        // the scalar chain: two v_rsq_f32 and one reciprocal.  1/|alpha| and gamma take a Newton step: errors of 1 ulp in all
        // three scalars leave H_k unitary to 1e-7 still, but coherently over the whole matrix, and cost 0.2 % of the bench bins
        // their one-step guard (tridiag_presolve_model.py).  H_k annihilates x exactly whatever ||x|| is taken to be.
        const float a2 = fmaf(alr, alr, ali * ali);
        const float nrm = n2 * __builtin_amdgcn_rsqf(n2);
        const float ra = rsq_full(fmaxf(a2, 1e-36f));
        const bool pha = a2 > 1e-36f;
        const float phr = pha ? alr * ra : 1.f, phi = pha ? ali * ra : 0.f;
        // n2 is a non-negative float in a scalar register: it orders as its bit pattern, and the test runs on the scalar unit
        const float gam = __float_as_uint(n2) > __builtin_bit_cast(unsigned, 4e-30f) ? rcp_full(fmaf(nrm, a2 * ra, n2)) : 0.f;
        e[k] = uniform_scalar(nrm);
        e2[k] = n2;
        // u_i in quad i: the column entry, plus phi ||x|| in row k + 1 (whose entry is alpha itself), zero in the rows <= k.  One
        // masked ||x|| and two FMAs: straight-line code (the nested select on the pair compiled to a branch over the quads, and a
        // packed operation scheduled across it lost its operand modifiers).  Then this lane's columns from quads jq + 4 t
        const float un = tp_keep(nrm, tp_lanes(15, 4 * k1));
        const CF vi = mk<float>(fmaf(phr, un, bx), fmaf(phi, un, by));
        f2v vj[4];
        by_column((f2v){vi.x, vi.y}, vj, t0);
        // delta_{k+1} = -delta_k phi_k (off the chain: it fills the permutes' wait)
        {
            const float ndr = fmaf(dli, phi, -dlr * phr), ndi = -fmaf(dlr, phi, dli * phr);
            dlr = ndr; dli = ndi;
            sdel[k1] = (f2v){dlr, dli};
        }
        // A u and Q u, one complex accumulator each: per slot acc += a[t] u.x and acc += (i a[t]) u.y, the operands read as they are
        // (the first slot multiplies: no zero to materialise; the last instruction of each chain is the compiler's, see tp_fma_iy)
        f2v p, uq;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < t0) continue;
            const f2v vx = {vj[t].x, vj[t].x};
            if (t == t0) { p = tp_mul_iy(a[t], vj[t]); uq = tp_mul_iy(q[t], vj[t]); }
            else { tp_fma_iy(p, a[t], vj[t]); tp_fma_iy(uq, q[t], vj[t]); }
            p = __builtin_elementwise_fma(a[t], vx, p);
            uq = __builtin_elementwise_fma(q[t], vx, uq);
        }
        float pr = p.x, pi = p.y, ur = uq.x, ui = uq.y;                                      // (A u)_i, (Q u)_i
        // four chains, stage by stage
        tp_dpp_add<0xB1>(pr); tp_dpp_add<0xB1>(pi); tp_dpp_add<0xB1>(ur); tp_dpp_add<0xB1>(ui);
        tp_dpp_add<0x4E>(pr); tp_dpp_add<0x4E>(pi); tp_dpp_add<0x4E>(ur); tp_dpp_add<0x4E>(ui);
        // w = p + kappa u with p = gamma A u and kappa = -gamma/2 u^H p (real: A is Hermitian)
        const float uau = tp_sum_quads(fmaf(pr, vi.x, pi * vi.y));
        const float kap = -0.5f * gam * gam * uau;
        const CF wi = mk<float>(fmaf(gam, pr, kap * vi.x), fmaf(gam, pi, kap * vi.y));
        const f2v tu = {gam * ur, gam * ui};                                                // gamma (Q u)_i
        f2v wj[4];
        by_column((f2v){wi.x, wi.y}, wj, t0);
        const f2v uv = {vi.x, vi.y}, wv = {wi.x, wi.y};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < t0) continue;
            // A -= u w^H + w u^H;  Q -= (gamma Q u) u^H: acc -= z conj(s) is acc -= z s.x and acc += (i z) s.y
            const f2v vx = {vj[t].x, vj[t].x}, wx = {wj[t].x, wj[t].x};
            tp_fma_iy(a[t], uv, wj[t]);
            a[t] = __builtin_elementwise_fma(-uv, wx, a[t]);
            tp_fma_iy(a[t], wv, vj[t]);
            a[t] = __builtin_elementwise_fma(-wv, vx, a[t]);                                  // the next reflector reads a[t] by DPP
            tp_fma_iy(q[t], tu, vj[t]);
            q[t] = __builtin_elementwise_fma(-tu, vx, q[t]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    {
        // The last reflector is a sign.  The column below the diagonal is the single element alpha = A[15][14] (lane 62, slot 3),
        // so u_0 = 2 alpha, gamma = 1 / (2 |alpha|^2) and H_14 = diag(1, ..., 1, -1): A[15][15] stays, Q's column 15 changes sign
        // and delta_15 = -delta_14 phi.  The two signs cancel in Q diag(delta): the column is left alone and delta_15 =
        // +delta_14 phi.  No products, no wave sum, no permute, no update; e2 stays non-zero.
        const float alr = tp_lane(a[3].x, 62), ali = tp_lane(a[3].y, 62);
        const float a2 = fmaf(alr, alr, ali * ali);
        const float n2 = fmaxf(a2, 1e-31f);
        const float ra = rsq_full(fmaxf(a2, 1e-36f));
        const bool pha = a2 > 1e-36f;
        const float phr = pha ? alr * ra : 1.f, phi = pha ? ali * ra : 0.f;
        e[N - 2] = uniform_scalar(n2 * __builtin_amdgcn_rsqf(n2));
        e2[N - 2] = uniform_scalar(n2);
        sdel[N - 1] = (f2v){fmaf(-dli, phi, dlr * phr), fmaf(dlr, phi, dli * phr)};
    }
    float d[N];                                                            // diagonal (wave-uniform)
#pragma unroll
    for (int m = 0; m < N; ++m) d[m] = uniform_scalar(tp_lane(a[m >> 2].x, 4 * m + (m & 3)));
#pragma unroll
    for (int t = 0; t < 4; ++t) {                                          // Q diag(delta) to LDS for the back-transform
        const f2v dq = sdel[jq + 4 * t];
        const f2v s = __builtin_elementwise_fma((f2v){-q[t].y, q[t].x}, (f2v){dq.y, dq.y}, q[t] * (f2v){dq.x, dq.x});
        fQ[i * LDQ + jq + 4 * t] = mk<float>(s.x, s.y);
    }
    stamp(4);

    // ---- 2. eigenvalue m = i by multisection.  C is positive semi-definite with ||C|| <= ||C||_F, so the spectrum lies in
    // [-1e-3, 1.001] ||C||_F
    const float nrmF = sqrtf(normS2);
    // Sturm count: the negative pivots of T - x I.  A zero pivot gives rcp = inf, the next pivot -inf (counted), rcp(-inf) = -0.
    // The sign bit of every pivot is shifted into one word (v_alignbit_b32: one instruction per pivot) and counted once.  It
    // differs from `qv < 0` on a pivot of -0 only, and a fused -e2 r + (d - x) rounds to -0 only from a negative value that
    // underflowed (e2 > 0, and d - x is -0 for d = -0, x = +0 alone): the sign bit is the sign of the pivot.  (The NumPy
    // model has counted sign bits all along.)
    auto sturm = [&](float x) {
        float qv = d[0] - x;
        unsigned sg = __float_as_uint(qv) >> 31;
#pragma unroll
        for (int m = 1; m < N; ++m) {
            qv = fmaf(-e2[m - 1], __builtin_amdgcn_rcpf(qv), d[m] - x);
            sg = __builtin_amdgcn_alignbit(sg, __float_as_uint(qv), 31);
        }
        return __builtin_popcount(sg);
    };
    float lo = -1e-3f * nrmF, hi;
    {
        // The wide first step: every quad still searches the same interval, so lane l counts the eigenvalues below
        // lo + (l + 1) (hi - lo) / 65, 64 distinct points.  The counts are monotone in the lane, and nb_m, the number of lanes whose
        // count is <= m, places eigenvalue m in the nb_m-th 65th of the interval.  One wave vote and a scalar population count per
        // eigenvalue; v_writelane puts nb_m into lane m of one register and a single crossbar trip hands quad i its own.
        const float wd = 1.002f * nrmF;
        const int cnt = sturm(fmaf(wd, (float)(lane + 1) * (1.f / 65.f), lo));
        int nbv = 0;
        tp_vote<0>(cnt, nbv);
        const float nb = (float)__builtin_amdgcn_ds_bpermute(i << 2, nbv);
        const float w65 = (1.f / 65.f) * wd;
        lo = fmaf(nb, w65, lo);
        hi = lo + w65;
    }
    // The quad steps: lane (i, jq) counts the eigenvalues below lo + (jq + 1) (hi - lo) / 5
    const float frac = 0.2f * (float)(jq + 1);
#pragma unroll 1
    for (int st = 0; st < kTpQuadSteps; ++st) {
        const float wd = hi - lo;
        const int cnt = sturm(fmaf(wd, frac, lo));
        // The points are monotone in jq, so the number nb of the quad's points at or below eigenvalue i places it: the new interval
        // is the nb-th fifth of the old one.  A quad sum (two v_add_f32_dpp) and three operations; the min / max over the quad of
        // the points themselves was sixteen instructions (a v_mov_b32_dpp and the canonicalising v_max_f32 of every operand).
        // The ends are re-formed from lo, to rounding: a fraction of the Sturm count's own error (kTpLamErr's floor).
        const float nb = tp_sum_quad((cnt <= i) ? 1.f : 0.f);
        const float w5 = 0.2f * wd;
        lo = fmaf(nb, w5, lo);
        hi = lo + w5;
    }
    // The inverse iteration below is one lane's work, and a quad would run it four times over.  Instead each lane of the quad takes
    // a shift of its own, the points 1/8, 3/8, 5/8 and 7/8 of the final interval, and the best of the four is kept: two more bits
    // of the eigenvalue at no instruction.
    const float lsh = fmaf(hi - lo, 0.125f + 0.25f * (float)jq, lo);
    stamp(13);

    // ---- 3. eigenvector i: two inverse-iteration steps on T - lsh I, unpivoted L D L^T (pivots kept at least 1e-9 ||C|| away from
    // zero), start vector ones + e_i, normalised after each step.  No reorthogonalisation: the refinement's E = V^H V - I takes it.
    // The pivots' reciprocals are the bare v_rcp_f32 (1 ulp): the factorisation only has to serve an iteration whose result the
    // refinement certifies, and 1-ulp noise on them leaves the model's one-step share where it is (99.67 % against 99.69 % over 32 768
    // bench bins, 99.66 % against 99.62 % over 8 192: inside the sampling error of either).
    float l[N - 1], rdg[N], xv[N];
    {
        const float tiny = 1e-9f * nrmF;
        float piv = d[0] - lsh;
#pragma unroll
        for (int m = 0; m < N; ++m) {
            if (m > 0) piv = fmaf(-e[m - 1], l[m - 1], d[m] - lsh);
            piv = copysignf(fmaxf(fabsf(piv), tiny), piv);
            rdg[m] = __builtin_amdgcn_rcpf(piv);
            if (m < N - 1) l[m] = e[m] * rdg[m];
        }
    }
    float nrm2 = 0.f;
#pragma unroll
    for (int m = 0; m < N; ++m) xv[m] = (m == i) ? 2.f : 1.f;         // distinct starts: a double eigenvalue gets two vectors
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if (it > 0) {
            const float s = rsq_full(nrm2);
#pragma unroll
            for (int m = 0; m < N; ++m) xv[m] *= s;
        }
#pragma unroll
        for (int m = 1; m < N; ++m) xv[m] = fmaf(-l[m - 1], xv[m - 1], xv[m]);      // L y = b
        xv[N - 1] *= rdg[N - 1];
#pragma unroll
        for (int m = N - 2; m >= 0; --m) xv[m] = fmaf(-l[m], xv[m + 1], xv[m] * rdg[m]);   // D L^T x = y
        nrm2 = 0.f;
#pragma unroll
        for (int m = 0; m < N; ++m) nrm2 = fmaf(xv[m], xv[m], nrm2);
    }
    // The lane whose second step grew the normalised vector most has the shift nearest the eigenvalue: it wins.  nrm2 is a sum of
    // squares, and non-negative floats order as their bit patterns do, so the quad maximum is two integer DPP stages (no
    // canonicalising moves).  3 - jq in the two lowest bits makes the four keys distinct, so exactly one lane wins and a tie goes
    // to the lowest jq; the comparison is unsigned, so a NaN of either sign wins and fails the gate below.
    const unsigned key = (__float_as_uint(nrm2) & ~3u) | (unsigned)(3 - jq);
    unsigned kmx = key;
    kmx = max(kmx, (unsigned)__builtin_amdgcn_update_dpp(0, (int)kmx, 0xB1, 0xf, 0xf, true));
    kmx = max(kmx, (unsigned)__builtin_amdgcn_update_dpp(0, (int)kmx, 0x4E, 0xf, 0xf, true));
    const bool win = key == kmx;
    const bool finite = nrm2 > 0.f && nrm2 < 3.0e38f;
    {
        const float s = rsq_full(nrm2);
#pragma unroll
        for (int m = 0; m < N; ++m) xv[m] *= s;
    }
    if (win) {
#pragma unroll
        for (int m = 0; m < N; ++m) fX[m * LDX + i] = xv[m];
    }
    // the winner's shift is the quad's eigenvalue: a quad sum of it and three zeros (exact; a NaN stays a NaN)
    const float lam = tp_sum_quad(win ? lsh : 0.f);
    stamp(14);
    // eigenvalues closer than 1e-5 ||C|| (none on the bench data) may leave nearly parallel vectors, and the double-sweep fall-back
    // after the refinement only orthonormalises V32: it cannot restore a direction V32 lacks.  Such a bin is not trusted (double
    // sweeps on C itself), like a rank-deficient one.  kTpApart is 1e-5 widened by the multisection's own error.  Two eigenvalues
    // that share a final interval may win with the same shift: their gap reads <= 0 and the bin goes the same way, rightly, their
    // true gap being under kTpFinal.  The gap to the next eigenvalue is one crossbar trip from quad i + 1 (quad 15 reads quad 0
    // and does not use it).
    const float gap = tp_from(lam, (lane + 4) & 63) - lam;
    const bool apart = i == N - 1 || gap > kTpApart * nrmF;
    // spread of the spectrum, as the one-sided solve's gate.  Quad i holds eigenvalue i and the multisection delivers them in
    // ascending order (the Sturm count is one function of x for all quads, and the shifts lie inside the intervals), so the smallest
    // is quad 0's and the largest quad 15's: two readlanes, no reduction.  Any NaN, a non-finite winning vector or a close pair fails
    // the gate: a NaN in quad 0 or 15 fails the comparison, one anywhere fails `lam == lam` (and leaves its own vector non-finite
    // and its neighbour's gap NaN).
    const float mn = tp_lane(lam, 0), mx = tp_lane(lam, 63);
    const bool ok = (mn >= 1e-3f * mx) && !__any((win && !finite) || !apart || !(lam == lam));
    wsync();

    // ---- 4. V32 = Q X on the f32 matrix cores (X is real: eight products)
    f4 re = {0, 0, 0, 0}, im = {0, 0, 0, 0};
    const int rc = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const CF qa = fQ[rc * LDQ + 4 * s + kq];
        const float xb = fX[(4 * s + kq) * LDX + rc];
        re = __builtin_amdgcn_mfma_f32_16x16x4f32(qa.x, xb, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_16x16x4f32(qa.y, xb, im, 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) v32[t] = mk<float>(re[t], im[t]);
    stamp(5);
    return ok;
}

// XT: element type of the fused input slabs (float2 = c64, double2 = c128: the float64 streaming front-end)
// DBG: the diagnostic instantiation.  It alone carries the run-time `debug_stop` tests and the in-kernel stage stamps (p.stamps);
// in the product instantiation `dstop` is the constant 0 and all of it folds away.  debug_stop: 1, 2, 3 return after stage 0, 1,
// 2; 4 skips the float32 pre-solve (double sweeps only); 5 always takes the guarded path (double sweeps after the pre-solve);
// 9 marks the bins by the refinement step they miss (status 8 / 16); 10 switches the refinement's guard off (results invalid).
// Any other value runs the whole kernel.
// HOPS: the launch covers several hops of a chunk (blockIdx.z = hop): every operand moves on by its byte stride per hop (scalar
// arithmetic on the argument block; the instantiations without it are untouched)
template <typename T, bool FUSED, typename XT, bool DBG, int GS = 1, bool HOPS = false>
__device__ __forceinline__ void gevd16m_body(const GevdParams& p, const int k, const bool z1, const int hop = 0) {
    const int dstop = DBG ? p.debug_stop : 0;
    // stage stamps (diagnostic build only): s_memtime of lane 0 at the stage boundaries, 8 per bin, into a buffer of their own
    auto stamp = [&](int i) {
        if constexpr (DBG) {
            if (p.stamps != nullptr && threadIdx.x == 0)
                p.stamps[((size_t)(z1 ? 1 : 0) * p.K + k) * 16 + i] = __builtin_amdgcn_s_memtime();
        }
    };
    stamp(0);
    if constexpr (DBG) { if (p.stamps != nullptr && threadIdx.x == 0) p.stamps[((size_t)(z1 ? 1 : 0) * p.K + k) * 16 + 15] = __builtin_amdgcn_s_memrealtime(); }
    // zone program of a two-zone launch (z1); the argument block itself stays in scalar registers
    auto at_hop = [&](const void* base, size_t stride) -> const char* {
        const char* b = static_cast<const char*>(base);
        if constexpr (HOPS) return b ? b + (size_t)hop * stride : b;
        else return b;
    };
    const XT* const pXB = reinterpret_cast<const XT*>(at_hop(z1 ? p.XB1 : p.XB, p.hop_X));
    const XT* const pXD = reinterpret_cast<const XT*>(at_hop(z1 ? p.XD1 : p.XD, p.hop_X));
    const XT* const pd = reinterpret_cast<const XT*>(at_hop(z1 ? p.d1 : p.d, p.hop_d));
    void* const pw = const_cast<char*>(at_hop(z1 ? p.w1 : p.w, p.hop_w));
    void* const plam = const_cast<char*>(at_hop(z1 ? p.lam1 : p.lam, p.hop_lam));
    int32_t* const pstatus = reinterpret_cast<int32_t*>(const_cast<char*>(at_hop(z1 ? p.status1 : p.status, p.hop_status)));
    using C = Cx<T>;
    __shared__ C sA[N * LD];       // R_B -> W R_B (float32; float64: the real tile G of C) -> C -> Q (eigenvectors of C) (-> X for U)
    __shared__ alignas(16) C sB[N * LD];   // R_D (float64 slabs: its real tile G) -> W = L^-1 (16 bytes: the pre-solve reads its scratch here by ds_read_b128)
    __shared__ C scol[2][N];       // (stage 1 keeps its columns in sB; the later stages' small arrays live here)
    __shared__ C swr[2][N];        // Cholesky: current row of W
    __shared__ C sr[N];
    __shared__ C scoef[N];
    // The Cholesky staging is dead after stage 1; the later stages' small arrays live in it, which keeps the
    // workgroup at 10 240 B of LDS = exactly 16 workgroups (4 waves per SIMD) per CU.
    T* const sLam = reinterpret_cast<T*>(&scol[0][0]);                 // [N]
    int* const sOrder = reinterpret_cast<int*>(&scol[1][0]);           // [N]
    T (*const srot)[4] = reinterpret_cast<T(*)[4]>(&swr[0][0]);        // Jacobi: (c, s.x, s.y) of the eight rotations of a round

    const int lane = threadIdx.x;
    int status = 0;
    // One wave is a long dependent chain; in the per-hop streaming pipeline the launch shares the chip with the next hop's
    // transforms, whose waves would otherwise take every other issue slot: this wave goes first.  (No effect when the kernel runs
    // alone.)  The chunked whole-signal path asks for the opposite (yield_issue): there the transforms are the longer chain.
    if (!p.yield_issue) __builtin_amdgcn_s_setprio(3);

    // ---------------- stage 0 ----------------
    if constexpr (FUSED) {
        const size_t slab = (size_t)k * p.M * N;
        if constexpr (DBG) {
            correlate16<T, XT, true>(pXB + slab, pd + (size_t)k * p.M, p.M, sA, sr, lane, stamp, 8);
            stamp(10);
            correlate16<T, XT, false>(pXD + slab, (const XT*)nullptr, p.M, sB, sr, lane, stamp, 11);
        } else if constexpr (GS > 1) {
            // grouped spectra [K / GS][M L][GS]: the bin's elements are GS apart, starting at its place inside the group
            const size_t gslab = (size_t)(k / GS) * p.M * N * GS + (k % GS);
            correlate16<T, XT, true, NoStamp, GS>(pXB + gslab, pd + (size_t)k * p.M, p.M, sA, sr, lane);
            correlate16<T, XT, false, NoStamp, GS>(pXD + gslab, (const XT*)nullptr, p.M, sB, sr, lane);
        } else {
            correlate16<T, XT, true>(pXB + slab, pd + (size_t)k * p.M, p.M, sA, sr, lane);
            correlate16<T, XT, false>(pXD + slab, (const XT*)nullptr, p.M, sB, sr, lane);
        }
    } else {
        const C* RB = reinterpret_cast<const C*>(p.RB) + (size_t)k * N * N;
        const C* RD = reinterpret_cast<const C*>(p.RD) + (size_t)k * N * N;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int idx = lane + 64 * t, i = idx >> 4, j = idx & 15;
            sA[i * LD + j] = RB[idx];
            sB[i * LD + j] = RD[idx];
        }
        if (lane < N) sr[lane] = p.r ? reinterpret_cast<const C*>(p.r)[(size_t)k * N + lane] : mk<T>(0, 0);
    }
    wsync();
    stamp(1);
    if (dstop == 1) return;

    // ---------------- stage 1: Cholesky of B + reg I with W = L^-1 ----------------
    // lane (i = lane>>2, jq = lane&3) owns B[i][jq+4t] and W[i][jq+4t], t = 0..3, in registers
    const int i = lane >> 2, jq = lane & 3;
    C brow[4], wrow[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = jq + 4 * t;
        if constexpr (FUSED && sizeof(T) == 8) {
            // float64 slabs: correlate16 left the real tile G of R_D in sB's real parts, and the row is un-mixed here, from G_ij and
            // G_ji, by the operations correlate16 applies to R_B: R_D = R_D^H bit for bit and Im R_D_ii = 0 exactly
            const T gij = sB[i * LD + j].x, gji = sB[j * LD + i].x;
            brow[t] = mk<T>((T)0.5 * (gij + gji), (T)0.5 * (gij - gji));
        } else {
            brow[t] = sB[i * LD + j];
        }
        if (j == i) brow[t] = mk<T>(brow[t].x + (T)p.reg_dark, 0);
        wrow[t] = mk<T>((j == i) ? (T)1 : (T)0, 0);
    }
    // Every step has a column buffer of its own in sB (R_D is in brow[] by now and W goes back there only after the loop): column
    // kk of the working B, pivot included, stays at ccol[kk] until the loop is over.  So the loop neither tests nor stores the
    // pivot: a step is one LDS round trip (pivot, column and row behind one wsync) and straight-line code, and the pivots are
    // tested afterwards, all sixteen at once.  After a bad pivot the remaining steps compute inf / NaN that nothing reads.
    C (*const ccol)[N] = reinterpret_cast<C(*)[N]>(&sB[0]);
    wsync();                                                                    // every lane has its row of R_D
#pragma unroll
    for (int kk = 0; kk < N; ++kk) {
        const int buf = kk & 1;
        if (jq == (kk & 3)) ccol[kk][i] = brow[kk >> 2];                        // column kk of the working B
        if (i == kk) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (4 * t <= kk) swr[buf][jq + 4 * t] = wrow[t];                // row kk of the working W (zero beyond column kk)
        }
        wsync();
        // all of the step's reads behind the one wsync: pivot, B[i][kk], the column entries and the row of W
        const T dkk = ccol[kk][kk].x;
        const C li = ccol[kk][i];
        C lj[4], wk[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (4 * t + 3 > kk) lj[t] = ccol[kk][jq + 4 * t];
            if (4 * t <= kk) wk[t] = swr[buf][jq + 4 * t];
        }
        // 1/d for the updates now; the 1/sqrt(d) that scales row kk of W is taken once, for all rows together, after the loop
        const T inv2 = rcp_full(dkk);
        const C li2 = mk<T>(li.x * inv2, li.y * inv2);
        // The outer-product update of B runs on the whole Hermitian matrix, without the triangle tests: rows and columns
        // already eliminated only cancel to rounding level and are never read again, and the unconditional update costs less
        // than its predicates.  W: rows past the pivot take the (unscaled) pivot row, which is zero beyond column kk.
        // What the unrolled loop knows at compile time is skipped: column groups of B entirely at or before the pivot
        // (4t + 3 <= kk) and groups of W entirely beyond it (4t > kk).
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (4 * t + 3 <= kk) continue;
            // B[i][j] -= B[i][kk] conj(B[j][kk]) / d
            // each component as two chained FMAs (written a -= p q + r s it compiles to a product, an FMA and a subtraction)
            brow[t].x = fma_t(-li2.y, lj[t].y, fma_t(-li2.x, lj[t].x, brow[t].x));
            brow[t].y = fma_t(li2.x, lj[t].y, fma_t(-li2.y, lj[t].x, brow[t].y));
        }
        if (i > kk) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (4 * t > kk) continue;
                // W[i][j] -= (B[i][kk] / d) W[kk][j]
                wrow[t].x = fma_t(li2.y, wk[t].y, fma_t(-li2.x, wk[t].x, wrow[t].x));
                wrow[t].y = fma_t(-li2.y, wk[t].x, fma_t(-li2.x, wk[t].y, wrow[t].y));
            }
        }
    }
    wsync();
    {
        // the pivots, each row's own: one bad one (not positive, NaN, or beyond 3e38) fails the bin
        const T di = ccol[i][i].x;
        if (__any(!(di > (T)0) || !(di < (T)3.0e38))) status = 1;
        if (status == 0) {
            // W = D^-1/2 (unit lower factor)^-1: every row by the reciprocal root of its pivot, one rsq for the sixteen rows at once
            // (inside the loop it was a serial rsq per step and a branch for the pivot row)
            const T ri = rsq_full(di);
#pragma unroll
            for (int t = 0; t < 4; ++t) wrow[t] = mk<T>(wrow[t].x * ri, wrow[t].y * ri);
        }
    }
    stamp(2);
    if (dstop == 2) return;

    if (status == 0) {
        // W -> sB (R_D is spent)
#pragma unroll
        for (int t = 0; t < 4; ++t) sB[i * LD + jq + 4 * t] = wrow[t];
        wsync();
        // ---------------- stage 2: C = W A W^H ----------------
        C acc[4];
        const int col = lane & 15;
        if constexpr (sizeof(T) == 8) {
            // float64: T1 = W A never goes to LDS.  The first product is formed transposed, X = T1^T = A^T W^T (both operands
            // read transposed: every real product multiplies the two numbers it always did, in the same k order, so X_ij has
            // the bits of T1_ji), and its accumulator X[(lane >> 4) + 4 t][lane & 15] is, k-step by k-step, the A operand T1 of
            // the second product.  That one is Hermitian, C = T1 W^H, and comes from its real tile G = Re C + Im C (hmm16_tile:
            // 8 MFMAs for the 12 of a general product, W fetched once).  G passes through sA (R_B is spent: every read of it
            // feeds the MFMAs G depends on) as a dense real tile of odd row stride, and C_ij = ((G_ij + G_ji) / 2,
            // (G_ij - G_ji) / 2): C = C^H bit for bit, Im C_ii = 0 exactly.
            cmm16([&](int r, int kx) { return sA[kx * LD + r]; }, [&](int kx, int c) { return sB[c * LD + kx]; }, lane, acc);
            const d4 g = hmm16_tile(acc, [&](int c, int kx) { return sB[c * LD + kx]; }, lane);
            T* const sG = reinterpret_cast<T*>(&sA[0]);
#pragma unroll
            for (int t = 0; t < 4; ++t) sG[mfma_row<T>(lane, t) * LDG + col] = g[t];
            wsync();
            T gt[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) gt[t] = sG[col * LDG + mfma_row<T>(lane, t)];
            wsync();
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = mk<T>((T)0.5 * (g[t] + gt[t]), (T)0.5 * (g[t] - gt[t]));
        } else {
            cmm16([&](int r, int kx) { return sB[r * LD + kx]; }, [&](int kx, int c) { return sA[kx * LD + c]; }, lane, acc);
            wsync();
#pragma unroll
            for (int t = 0; t < 4; ++t) sA[mfma_row<T>(lane, t) * LD + col] = acc[t];          // T1 = W A
            wsync();
            cmm16([&](int r, int kx) { return sA[r * LD + kx]; },
                  [&](int kx, int c) { const C w = sB[c * LD + kx]; return mk<T>(w.x, -w.y); }, lane, acc);
            wsync();
        }
        T nrm = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int row = mfma_row<T>(lane, t);
            if (sizeof(T) != 8 && row == col) acc[t].y = 0;                                // (float64: zero already, from the tile)
            sA[row * LD + col] = acc[t];                                                    // C
            nrm += acc[t].x * acc[t].x + acc[t].y * acc[t].y;
        }
        // (wave-uniform: kept in scalar registers -- the vector registers of this kernel are all spoken for; as a vector value the
        // scaled norm was spilled on the common path, 8 bytes per lane = 17 MB of scratch written per launch)
        // float64: the butterfly on the VALU (wave_sum_valu: the same additions in the same order, and every lane holds the total)
        T normF2;
        if constexpr (sizeof(T) == 8) normF2 = uniform_scalar(wave_sum_valu(nrm));
        else normF2 = uniform_scalar(wave_sum(nrm));
        wsync();
        stamp(3);
        if (dstop == 3) return;

        // ---------------- stage 3: register-resident Jacobi, XOR schedule ----------------
        const int a = lane >> 3, b = lane & 7;
        const int max_sweeps = p.max_sweeps > 0 ? p.max_sweeps : Prec<T>::max_sweeps;
        const T tol2 = p.sweep_tol2 > 0.0 ? (T)p.sweep_tol2 : Prec<T>::sweep_tol2;
        bool converged = false;
        // the scale exponent is wave-uniform: kept in a scalar register, the factors are re-formed where they are used
        const int sexp = __builtin_amdgcn_readfirstlane((normF2 > (T)0) ? -((sizeof(T) == 8 ? ilogb((double)normF2) : ilogbf((float)normF2)) / 2) : 0);
        T normS2;
        if constexpr (sizeof(T) == 8) normS2 = uniform_scalar((T)ldexp((double)normF2, 2 * sexp));
        else normS2 = uniform_scalar((T)ldexpf((float)normF2, 2 * sexp));
        bool v_in_lds = false, refined = false;
        // float64, first refinement step: does the launch read eigenvector columns beyond the eight leading ones?  (Uniform over
        // the launch but for the diagnostic stops.)  Ranks above 8, the eigenvalue or eigenvector outputs, a contrast floor (its
        // c_v run over all sixteen terms; mu and the cap of a span only ever shorten the list), and the diagnostic stops that
        // mark or time the whole step.  keep_a: the leading half passed its guard and the other did not -- its columns (qa: one
        // component of four elements per lane) and eigenvalues wait for the guarded path to end.
        const bool need_b = p.ranks[p.nV - 1] > 8 || p.lam != nullptr || p.lam1 != nullptr || p.U != nullptr ||
                            (p.span.on && p.span.phi > 0.0) || (DBG && (dstop == 9 || dstop == 5 || dstop == 10));
        bool keep_a = false;
        T qa[4] = {0, 0, 0, 0};
        T* const sLamA = sLam + N;                                            // [8] half A's eigenvalues meanwhile (free half of scol[0])
        // A one-sided solve is used only if it converged and its eigenvalues (the squared column norms) span less than 1e3: its
        // stop criterion is absolute, so columns of smaller norm (the null space of a rank-deficient C sits at the shift) may be
        // left askew.  Such a bin takes the two-sided sweeps on C, which is still intact in sA at that point.
        auto spectrum_ok = [&](float nt, float nb) {
            float mn = fminf(nt, nb), mx = fmaxf(nt, nb);
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {                                    // over the wave (any lane layout)
                mn = fminf(mn, __shfl_xor(mn, m, 64));
                mx = fmaxf(mx, __shfl_xor(mx, m, 64));
            }
            return !__any(!(mn >= 1e-3f * mx));                                   // NaN counts as not ok
        };
        if constexpr (sizeof(T) == 8) {
            // ---- float32 pre-solve (debug_stop == 4 skips it: double sweeps only, for A/B timing) -------------------
            // Double sweeps would be the cost of the kernel, so C is first diagonalised in float32: V32 with V32^H C V32 diagonal
            // to ~1e-7.  V32 is then refined against the exact float64 C on
            // the matrix cores (below); W waits in registers meanwhile.
            if (dstop != 4) {
                using CF = Cx<float>;
                CF v32[4];
                // Householder tridiagonal, multisection and inverse iteration (tridiag_presolve16); its scratch is sB, free until V32
                // lands there (W waits in registers)
                CF* const fQ = reinterpret_cast<CF*>(&sB[0]);
                const bool trust = tridiag_presolve16<T>(sA, sexp, (float)normS2, fQ, reinterpret_cast<float*>(fQ + N * LDQ), lane, v32, stamp);
                if (!trust) {
                    wsync();
#pragma unroll
                    for (int t = 0; t < 4; ++t) sB[i * LD + jq + 4 * t] = wrow[t];      // the pre-solve's scratch went through sB: W back in place
                    wsync();
                } else {
                const int mcol = lane & 15;
                auto cj = [](C w) { return mk<T>(w.x, -w.y); };
                wsync();
#pragma unroll
                for (int t = 0; t < 4; ++t) sB[mfma_row<float>(lane, t) * LD + mcol] = mk<T>((T)v32[t].x, (T)v32[t].y);   // V32 takes W's place
                wsync();
                C accT[4];
                cmm16([&](int r, int kx) { return sA[r * LD + kx]; }, [&](int kx, int c) { return sB[kx * LD + c]; }, lane, accT);       // C V
                // ---- one refinement step on the matrix cores in place of the double sweep (Ogita & Aishima 2018) ---------
                // With S = V^H C V, Gram = V^H V = I + E and the Rayleigh quotients d_i = S_ii / Gram_ii, the update
                //   V'' = V (I + Z),  Z_ij = (S_ij - d_j E_ij) / (d_j - d_i)  (i != j),  Z_ii = -E_ii / 2
                // removes the float solve's error to second order: what is left is |Z|^2, the same order a double Jacobi sweep
                // from (C', V') leaves.  |Z_ij| <= kRefineGuard on every pair keeps that below 1e-9; a wave that meets a
                // narrower spectral gap (or a pair the pre-solve did not resolve) takes the double sweeps instead.
                constexpr double kRefineGuard2 = 9e-10;        // |Z_ij|^2 <= (3e-5)^2
                // A step that misses the guard by less than |Z_ij| <= 1e-2 is applied all the same and followed by a second one
                // in the rotated basis: S'' = (I+Z)^H S (I+Z) needs no C (the accumulator of S is itself an MFMA operand),
                // Gram'' = V''^H V''.  On the bench workload 24 % of the bins miss the guard at the first step (two eigenvalues
                // closer than ~3e-3 ||C||) and all but 0.1 % pass it at the second; the double sweeps are left for true clusters.
                constexpr double kSecondStep2 = 1e-4;
                // debug_stop == 5: always the double sweeps (A/B timing); a caller-set sweep tolerance (jdiag: 1e-17) asks for more
                // than the refinement's 1e-9 and gets the sweeps too
                const bool refine_ok = (dstop != 5) && !(p.sweep_tol2 > 0.0);
                // Z goes straight into sA (T = C V is spent: every lane is past the third product) and the second-order
                // eigenvalue terms into the idle coefficient array: nothing of this step stays in registers
                T* const sLam2 = reinterpret_cast<T*>(&scoef[0]);
                // ---- the first step from the residual: one float64 product and two float32 ones -------------------
                // Off the diagonal the step needs S and Gram only through S_ij - d_j E_ij = (V^H (C V - V D))_ij.  The residual
                // Rs = T - V D, formed element by element in float64, carries the whole cancellation (it is ~1e-6 ||C|| after the
                // float32 pre-solve); V^H Rs and V Z then need relative accuracy only and run as float32 products (V is
                // float32-valued exactly here, |Z| <= 3e-5).  On the diagonal d_j = (v_j^H t_j) / g_j and g_j = v_j^H v_j are
                // sixteen column dot products.  A bin that misses the guard has lost nothing: T is still in accT, V in sB, and the
                // float64 products below start from them as they always did.
                if (refine_ok) {
                    // The step runs in two halves of eight columns ("The leading half alone"): half A = columns
                    // 8..15, the eight leading eigenvectors (the pre-solve delivers ascending eigenvalues), half B = columns 0..7,
                    // only for a launch that reads them.  A half's Rs and Z are real 16 x 16 float tiles [re | im] and its two
                    // products packed ones (pmm16): 8 MFMAs where the full complex product takes 16.
                    constexpr int LDR = 17;
                    float* const fT = reinterpret_cast<float*>(&sA[0]);   // tiles Rs, Z of half A, then of half B: 4 x 16 x 17 x 4 B
                                                                          // = all of sA; C is spent once T is in registers
                    T* const sG = reinterpret_cast<T*>(&scol[1][0]) + 8;  // [N] column norms g_j, behind sOrder's place
                    const bool lo = (lane & 8) == 0;                      // this lane's tile column holds real parts
                    const T scl = (T)ldexp(1.0, sexp);                  // the pre-solve's scale: Rs 2^sexp is ~1e-6 whatever ||C|| is
                    C vv[4];
                    T num = (T)0, g = (T)0;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        vv[t] = sB[mfma_row<T>(lane, t) * LD + mcol];
                        num = __builtin_fma(vv[t].y, accT[t].y, __builtin_fma(vv[t].x, accT[t].x, num));
                        g = __builtin_fma(vv[t].y, vv[t].y, __builtin_fma(vv[t].x, vv[t].x, g));
                    }
                    // the column's sixteen rows sit in this lane's four slots and in lanes ^ 16, ^ 32; every lane divides
                    rows_sum2_all(num, g);
                    T ginv = __builtin_amdgcn_rcp(g);
                    ginv = ginv * __builtin_fma(-g, ginv, (T)2);
                    T dj = num * ginv;
                    dj = __builtin_fma(__builtin_fma(-g, dj, num), ginv, dj);
                    if (lane < N) { sLam[mcol] = dj; sG[mcol] = g; }
                    wsync();                                            // every lane is past the product that read C
                    // Rs of both halves in one pass: a lane's column belongs to one of them (without half B its lanes store nothing)
                    if (need_b || !lo) {
                        float* const tR = fT + (lo ? 2 * N * LDR : 0) + (mcol & 7);
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const T rx = __builtin_fma(-vv[t].x, dj, accT[t].x) * scl, ry = __builtin_fma(-vv[t].y, dj, accT[t].y) * scl;
                            tR[mfma_row<T>(lane, t) * LDR] = (float)rx;
                            tR[mfma_row<T>(lane, t) * LDR + 8] = (float)ry;
                        }
                    }
                    wsync();
                    // One half up to its Z tile and eigenvalues (sLam2); true if it misses the guard.  The lane holds the real
                    // (lo) or the imaginary parts of four entries of column j: the formulas are those of the full step, |Z_ij|^2
                    // takes the other part's square from lane ^ 8 and is summed as zx zx + (zy zy) in the lanes of the real parts,
                    // which alone judge the guard and sum the eigenvalue's second-order term.
                    auto half_step = [&](const int h) -> bool {
                        const float* const tR = fT + (h ? 0 : 2 * N * LDR);
                        float* const tZ = fT + (h ? 1 : 3) * N * LDR;
                        const int j = 8 * h + (lane & 7);
                        float accP[4];
                        pmm16<false>([&](int r, int kx) { const C v = sB[kx * LD + r]; return mk<float>((float)v.x, (float)v.y); },
                                     [&](int kx, int c) { return tR[kx * LDR + c]; }, lane, accP);                                       // V^H Rs
                        const T djh = sLam[j];
                        const T zd = lo ? (T)0.5 * ((T)1 - sG[j]) : (T)0;
                        bool bad = false;
                        T l2 = (T)0;
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int row = mfma_row<float>(lane, t);
                            const bool offd = row != j;
                            const T den = djh - sLam[row], dens = den * scl;
                            T inv = __builtin_amdgcn_rcp(dens);
                            inv = inv * __builtin_fma(-dens, inv, (T)2);
                            const T z = (T)accP[t] * inv;
                            const T sq = z * z;
                            const T zz = __builtin_fma(z, z, dpp_xor8(sq));
                            bad = bad || (offd && lo && !(zz <= (T)kRefineGuard2));      // NaN / inf count as bad
                            l2 = offd ? __builtin_fma(zz, den, l2) : l2;                 // the eigenvalue's second-order term, as below
                            tZ[row * LDR + mcol] = (float)(offd ? z : zd);
                        }
                        l2 = rows_sum(l2);
                        if (lane < 8) sLam2[j] = l2 + djh;
                        return __any(bad) && dstop != 10;
                    };
                    bool miss = half_step(1), miss_b = false;
                    if (need_b && !miss) miss_b = half_step(0);
                    wsync();
                    if (!miss && !need_b) {
                        // the leading eight must come from half A: all 64 pairs (column of A, column of B), one per lane
                        miss = __any(!(sLam2[8 + (lane & 7)] > sLam[lane >> 3]));
                    }
                    if (!miss) {
                        float accZ[4];
                        auto vr = [&](int r, int kx) { const C v = sB[r * LD + kx]; return mk<float>((float)v.x, (float)v.y); };
                        pmm16<true>(vr, [&](int kx, int c) { return fT[N * LDR + kx * LDR + c]; }, lane, accZ);                         // V Z
                        T qb[4];
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            // this lane's component of V[row][lane & 7] and V[row][8 + (lane & 7)]
                            const T* const v = reinterpret_cast<const T*>(&sB[mfma_row<float>(lane, t) * LD + (lane & 7)]) + (lo ? 0 : 1);
                            qa[t] = v[2 * 8] + (T)accZ[t];                              // V'' = V + V Z, added in float64
                            qb[t] = v[0];                                               // without half B: the V32 values
                        }
                        if (miss_b) {
                            // the other half goes the guarded path below, which takes all sixteen columns as it always did;
                            // this half's results wait and take their columns back afterwards
                            if (lane < 8) sLamA[lane] = sLam2[8 + lane];
                            keep_a = true;
                        } else {
                            if (need_b) {
                                pmm16<true>(vr, [&](int kx, int c) { return fT[3 * N * LDR + kx * LDR + c]; }, lane, accZ);             // V Z
#pragma unroll
                                for (int t = 0; t < 4; ++t) qb[t] += (T)accZ[t];
                            }
                            if (lane < N && (need_b || lane >= 8)) sLam[lane] = sLam2[lane];
                            wsync();
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                T* const q = reinterpret_cast<T*>(&sA[mfma_row<float>(lane, t) * LD + (lane & 7)]) + (lo ? 0 : 1);
                                q[0] = qb[t];                                            // Q for stage 5; sLam holds the eigenvalues
                                q[2 * 8] = qa[t];
                                sB[i * LD + jq + 4 * t] = wrow[t];                      // W back in place for stage 5
                            }
                            wsync();
                            refined = true;
                        }
                    }
                }
                if (!refined) {
                // ---- the guarded path: the step in float64 throughout, the second step, the double sweeps ----------------------
                C accG[4], accC[4], accV[4];
                cmm16([&](int r, int kx) { return cj(sB[kx * LD + r]); }, [&](int kx, int c) { return sB[kx * LD + c]; }, lane, accG);   // V^H V
                wsync();
#pragma unroll
                for (int t = 0; t < 4; ++t) sA[mfma_row<T>(lane, t) * LD + mcol] = accT[t];
                wsync();
                cmm16([&](int r, int kx) { return cj(sB[kx * LD + r]); }, [&](int kx, int c) { return sA[kx * LD + c]; }, lane, accC);   // C1 = V^H C V
                for (int step = 0; step < 2; ++step) {
                    {
                        // Rayleigh quotients S_jj / Gram_jj of the sixteen lanes that hold a diagonal element: the element is
                        // selected first and divided once, by reciprocal, Newton step and one residual correction (a double
                        // division per accumulator row under its own branch was ~150 instructions of this step)
                        T num = (T)0, gd = (T)1;
                        bool has_diag = false;
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const bool d = mfma_row<T>(lane, t) == mcol;
                            num = d ? accC[t].x : num;
                            gd = d ? accG[t].x : gd;
                            has_diag = has_diag || d;
                        }
                        T ginv = __builtin_amdgcn_rcp(gd);
                        ginv = ginv * __builtin_fma(-gd, ginv, (T)2);
                        T quot = num * ginv;
                        quot = __builtin_fma(__builtin_fma(-gd, quot, num), ginv, quot);
                        if (has_diag) sLam[mcol] = quot;
                    }
                    wsync();
                    bool bad = false, hopeless = false;
                    const T dj = sLam[mcol];
                    T l2 = (T)0;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int row = mfma_row<T>(lane, t);
                        const T di = sLam[row];
                        C z;
                        if (row == mcol) {
                            z = mk<T>((T)0.5 * ((T)1 - accG[t].x), (T)0);
                        } else {
                            const T den = dj - di;
                            T inv = __builtin_amdgcn_rcp(den);
                            inv = inv * __builtin_fma(-den, inv, (T)2);                  // one Newton step: full precision
                            const T zx = __builtin_fma(-dj, accG[t].x, accC[t].x) * inv, zy = __builtin_fma(-dj, accG[t].y, accC[t].y) * inv;
                            const T zz = zx * zx + zy * zy;
                            bad = bad || !(zz <= (T)kRefineGuard2);                      // NaN / inf (equal quotients) count as bad
                            hopeless = hopeless || !(zz <= (T)kSecondStep2);
                            z = mk<T>(zx, zy);
                            // second-order term of the eigenvalue of the pencil (S, Gram) next to d_j, summed by COLUMNS: S and E are
                            // Hermitian, so row i gives eigenvalue j the term |S_ij - d_j E_ij|^2 / (d_j - d_i) = |Z_ij|^2 (d_j - d_i),
                            // one FMA on what the guard has formed already.  (Exact to third order in Z AND E: a float32 pre-solve
                            // can leave E ~ 1e-5 between the columns of small eigenvalues, where a formula that orthonormalises to
                            // first order only is off by E^2.)  Equal quotients give NaN: such a step is `bad` and never reads it.
                            l2 = __builtin_fma(zz, den, l2);
                        }
                        sA[row * LD + mcol] = z;
                    }
                    // the column's sixteen rows sit in this lane's four slots and in lanes ^ 16, ^ 32; then add the quotient itself
                    l2 = rows_sum(l2);
                    if (lane < N) sLam2[mcol] = l2 + dj;
                    const bool pass = !__any(bad) || dstop == 10;                 // 10: guard off (timing aid, results invalid)
                    if (dstop == 9 && !pass) status = 8 << step;                  // 9: mark the bins by the step they miss
                    // the double sweeps start from the triple (V, S, Gram) as it is: leave before anything of it is touched
                    if (!refine_ok || (!pass && (step == 1 || __any(hopeless)))) break;
                    wsync();
                    auto v_step = [&]() {
                        cmm16([&](int r, int kx) { return sB[r * LD + kx]; }, [&](int kx, int c) { return sA[kx * LD + c]; }, lane, accV);   // V Z
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const C v = sB[mfma_row<T>(lane, t) * LD + mcol];
                            accV[t] = mk<T>(v.x + accV[t].x, v.y + accV[t].y);                                                               // V'' = V (I + Z)
                        }
                    };
                    if (pass) {
                        v_step();
                        if (lane < N) sLam[lane] = sLam2[lane];
                        wsync();
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            sA[mfma_row<T>(lane, t) * LD + mcol] = accV[t];             // Q for stage 5; sLam already holds the eigenvalues
                            sB[i * LD + jq + 4 * t] = wrow[t];                          // W back in place for stage 5
                        }
                        wsync();
                        refined = true;
                        break;
                    }
                    if constexpr (sizeof(T) == 8) {
                        // the triple after the step.  P = S (I + Z) takes S^T = conj(S) from its accumulator as the A operand,
                        // S'' = (I + Z)^H P takes P's accumulator as the B operand; then V'' and its Gram matrix
                        auto ipz = [&](int r, int c) { const C zv = sA[r * LD + c]; return mk<T>(zv.x + (r == c ? (T)1 : (T)0), zv.y); };
                        cmm16x([&](int s_, int, int) { return cj(accC[s_]); }, [&](int, int kx, int c) { return ipz(kx, c); }, lane, accT);           // P
                        cmm16x([&](int, int r, int kx) { return cj(ipz(kx, r)); }, [&](int s_, int, int) { return accT[s_]; }, lane, accC);          // S''
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            if (mfma_row<T>(lane, t) == mcol) accC[t].y = 0;
                        v_step();
                        wsync();
#pragma unroll
                        for (int t = 0; t < 4; ++t) sB[mfma_row<T>(lane, t) * LD + mcol] = accV[t];                                      // V''
                        wsync();
                        cmm16([&](int r, int kx) { return cj(sB[kx * LD + r]); }, [&](int kx, int c) { return sB[kx * LD + c]; }, lane, accG);   // Gram''
                    }
                }
                if (!refined) {
                    // ---- double sweeps instead ----------------------------------------------------------------------------------
                    // They start from an orthonormal V' and C' = V'^H C V'.  V' = V Y with Y = I - E/2 = (3 I - Gram)/2 is
                    // orthonormal to E^2 and C' = Y S Y exactly (Y is Hermitian; S and the intermediate product feed the MFMA
                    // from their accumulators).  A trusted pre-solve leaves |E| of a few 1e-2 at worst (one large eigenvalue and a cluster
                    // at 1.5e-3 of it: 3e-2 in the NumPy model), so four steps do with room to spare: 1e-1 -> 7.5e-3 -> 4e-5 -> 1e-9 -> 1e-18.
                    constexpr int n_it = 4;
                    {
                    for (int it = 0; it < n_it; ++it) {
                        wsync();
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int row = mfma_row<T>(lane, t);
                            sA[row * LD + mcol] = mk<T>((row == mcol ? (T)1.5 : (T)0) - (T)0.5 * accG[t].x, (T)-0.5 * accG[t].y);      // Y
                        }
                        wsync();
                        cmm16([&](int r, int kx) { return sB[r * LD + kx]; }, [&](int kx, int c) { return sA[kx * LD + c]; }, lane, accV);   // V Y
                        cmm16x([&](int s_, int, int) { return cj(accC[s_]); }, [&](int, int kx, int c) { return sA[kx * LD + c]; }, lane, accT);   // S Y
                        cmm16x([&](int, int r, int kx) { return sA[r * LD + kx]; }, [&](int s_, int, int) { return accT[s_]; }, lane, accC);       // Y (S Y)
                        wsync();
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            sB[mfma_row<T>(lane, t) * LD + mcol] = accV[t];                                                              // V'
                            if (mfma_row<T>(lane, t) == mcol) accC[t].y = 0;
                        }
                        wsync();
                        if (it + 1 < n_it)
                            cmm16([&](int r, int kx) { return cj(sB[kx * LD + r]); }, [&](int kx, int c) { return sB[kx * LD + c]; }, lane, accG);   // Gram'
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) sA[mfma_row<T>(lane, t) * LD + mcol] = accC[t];                                          // C'
                    wsync();
                    }
                    v_in_lds = true;
                }
                }
                }
            }
        }
        if constexpr (sizeof(T) == 4) {
            // float kernel: the one-sided form IS the solve.  Eigenvalues are the squared column norms less the shift, eigenvectors
            // the normalised columns.
            constexpr int LDF = 17;
            constexpr float kShift = 8e-6f;
            const float delta = kShift * sqrtf((float)normS2);
            Cx<float>* const fG = reinterpret_cast<Cx<float>*>(&sB[0]);
            Cx<float> (*const fcol)[16] = reinterpret_cast<Cx<float>(*)[16]>(&scol[0][0]);
            chol16_f32<T, LD, LDF>(sA, sexp, delta, fG, fcol, lane);
            const int oa = lane & 7, ob = lane >> 3;                        // the one-sided solve's layout: lane = a + 8 b
            Cx<float> g0t = fG[(2 * oa) * LDF + ob], g0b = fG[(2 * oa) * LDF + 8 + ob];
            Cx<float> g1t = fG[(2 * oa + 1) * LDF + ob], g1b = fG[(2 * oa + 1) * LDF + 8 + ob];
            float n2t, n2b;
            (void)jacobi16_onesided<LDF>(g0t, g0b, g1t, g1b, lane, (float)tol2, (float)normS2, max_sweeps, converged, n2t, n2b, fG);
            const bool trust = converged && spectrum_ok(n2t, n2b);
            converged = false;
            wsync();
#pragma unroll
            for (int t = 0; t < 4; ++t) sB[i * LD + jq + 4 * t] = wrow[t];          // W back in place (stage 5, or the sweeps below)
            if (trust) {
                const int it_b = os_top_end(ob), ib_b = os_bot_end(ob);
                wsync();
                sA[(2 * oa) * LD + it_b] = mk<T>(g0t.x, g0t.y);
                sA[(2 * oa) * LD + ib_b] = mk<T>(g0b.x, g0b.y);
                sA[(2 * oa + 1) * LD + it_b] = mk<T>(g1t.x, g1t.y);
                sA[(2 * oa + 1) * LD + ib_b] = mk<T>(g1b.x, g1b.y);
                if (oa == 0) {
                    sLam[it_b] = (T)ldexpf(n2t - delta, -sexp);
                    sLam[ib_b] = (T)ldexpf(n2b - delta, -sexp);
                }
                refined = true;
            }
            wsync();
        }
        if (!refined) {
            C tt = sA[a * LD + b], tb = sA[a * LD + 8 + b], bt = sA[(8 + a) * LD + b], bb = sA[(8 + a) * LD + 8 + b];
            const T scl = (sizeof(T) == 8) ? (T)ldexp(1.0, sexp) : (T)ldexpf(1.0f, sexp);
            tt = mk<T>(tt.x * scl, tt.y * scl); tb = mk<T>(tb.x * scl, tb.y * scl);
            bt = mk<T>(bt.x * scl, bt.y * scl); bb = mk<T>(bb.x * scl, bb.y * scl);
            C v0t = mk<T>((2 * a == b) ? (T)1 : (T)0, 0), v0b = mk<T>((2 * a == 8 + b) ? (T)1 : (T)0, 0);
            C v1t = mk<T>((2 * a + 1 == b) ? (T)1 : (T)0, 0), v1b = mk<T>((2 * a + 1 == 8 + b) ? (T)1 : (T)0, 0);
            if (v_in_lds) {
                v0t = sB[(2 * a) * LD + b]; v0b = sB[(2 * a) * LD + 8 + b];
                v1t = sB[(2 * a + 1) * LD + b]; v1b = sB[(2 * a + 1) * LD + 8 + b];
                wsync();
    #pragma unroll
                for (int t = 0; t < 4; ++t) sB[i * LD + jq + 4 * t] = wrow[t];          // W back in place for stage 5
            }
            const bool diag = (a == b);
            const int sweeps_done = jacobi16_sweeps<T>(tt, tb, bt, bb, v0t, v0b, v1t, v1b, srot, lane, tol2, normS2, max_sweeps, converged);
            if (!converged) status = 2;
            // after an odd number of sweeps slot s holds (2s, 2s+1), after an even number (s, 8+s)
            const bool nat = sweeps_done & 1;
            const int it_b = nat ? 2 * b : b, ib_b = nat ? 2 * b + 1 : 8 + b;
            wsync();
            sA[(2 * a) * LD + it_b] = v0t;
            sA[(2 * a) * LD + ib_b] = v0b;
            sA[(2 * a + 1) * LD + it_b] = v1t;
            sA[(2 * a + 1) * LD + ib_b] = v1b;
            if (diag) {
                const T iscl = (sizeof(T) == 8) ? (T)ldexp(1.0, -sexp) : (T)ldexpf(1.0f, -sexp);
                sLam[it_b] = tt.x * iscl;
                sLam[ib_b] = bb.x * iscl;
            }
            wsync();
        }

        if constexpr (sizeof(T) == 8) {
            if (keep_a) {
                // the leading half's columns and eigenvalues from the fast step (the guarded path, sweeps included, keeps every
                // column at its index)
                wsync();
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    reinterpret_cast<T*>(&sA[mfma_row<float>(lane, t) * LD + 8 + (lane & 7)])[(lane & 8) ? 1 : 0] = qa[t];
                if (lane < 8) sLam[8 + lane] = sLamA[lane];
                wsync();
            }
        }
        stamp(6);
        // ---------------- stage 4: descending order ----------------
        // all 64 lanes: lane (i = lane & 15, q = lane >> 4) compares eigenvalue i with four others, the counts meet over q
        {
            const int i16 = lane & 15, q4 = lane >> 4;
            const T li = sLam[i16];
            int rank = 0;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = 4 * q4 + jj;
                const T lj = sLam[j];
                rank += (lj > li) || (lj == li && j < i16);
            }
            if constexpr (sizeof(T) == 8) rank = rows_sum(rank);
            else { rank += __shfl_xor(rank, 16, 64); rank += __shfl_xor(rank, 32, 64); }
            if (q4 == 0) sOrder[rank] = i16;
        }

        // ---------------- stage 5: g = W r ----------------
        // The filter needs X = W^H Q only through x_i^H r = q_i^H (W r) and sum a_i x_i = W^H (sum a_i q_i): two matrix-vector
        // products in place of the 16 x 16 x 16 one (which is formed at the very end, and only for a caller that asks for U).
        // all 64 lanes: lane (i, q) sums four of the sixteen terms of row i of W, the partial sums meet over q; g takes r's place
        {
            const int i16 = lane & 15, q4 = lane >> 4;
            T gx = 0, gy = 0;
#pragma unroll
            for (int ll = 0; ll < 4; ++ll) {
                const int l = 4 * q4 + ll;
                const C w = sB[i16 * LD + l], rr = sr[l];
                gx = fma_t(-w.y, rr.y, fma_t(w.x, rr.x, gx));
                gy = fma_t(w.y, rr.x, fma_t(w.x, rr.y, gy));
            }
            if constexpr (sizeof(T) == 8) {
                // the partial sums meet on the VALU (rows_sum2): row 0 holds the real part and row 1 the imaginary part, and each
                // stores its own
                const T s = rows_sum2(gx, gy);
                wsync();                                                    // every lane has read r
                if (q4 < 2) reinterpret_cast<T*>(&sr[i16])[q4] = s;
            } else {
                gx += __shfl_xor(gx, 16, 64); gy += __shfl_xor(gy, 16, 64);
                gx += __shfl_xor(gx, 32, 64); gy += __shfl_xor(gy, 32, 64);
                wsync();                                                    // every lane has read r
                if (q4 == 0) sr[i16] = mk<T>(gx, gy);
            }
        }
        wsync();

        // ---------------- stage 6: coefficients (x_i^H r) / (lam_i + mu) = (q_i^H g) / (lam_i + mu) ----------------
        // all 64 lanes: lane (i, q) sums four of the sixteen terms of q_i^H g, the partial sums meet over q
        {
            const int i16 = lane & 15, q4 = lane >> 4;
            T sx = 0, sy = 0;
#pragma unroll
            for (int ll = 0; ll < 4; ++ll) {
                const int l = 4 * q4 + ll;
                const C v = sA[l * LD + i16], rr = sr[l];
                sx = fma_t(v.y, rr.y, fma_t(v.x, rr.x, sx));
                sy = fma_t(-v.y, rr.x, fma_t(v.x, rr.y, sy));
            }
            if constexpr (sizeof(T) == 8) {
                const T s = rows_sum2(sx, sy);                              // as in stage 5: rows 0 and 1 scale and store a part each
                if (q4 < 2) {
                    const T den = rcp_full(sLam[i16] + span_mu<true, T>(p.span, z1, k, p.mu));
                    reinterpret_cast<T*>(&scoef[i16])[q4] = s * den;
                }
            } else {
                sx += __shfl_xor(sx, 16, 64); sy += __shfl_xor(sy, 16, 64);
                sx += __shfl_xor(sx, 32, 64); sy += __shfl_xor(sy, 32, 64);
                if (q4 == 0) {
                    const T den = rcp_full(sLam[i16] + span_mu<true, T>(p.span, z1, k, p.mu));
                    scoef[i16] = mk<T>(sx * den, sy * den);
                }
            }
        }
        wsync();
    }

    // ---------------- outputs ----------------
    // all 64 lanes: lane (i = lane & 15, q = lane >> 4) sums the terms of the sorted columns q, q + 4, ... of element i of
    // y = sum a_c q_c, carried on from rank to rank; per rank the four partial sums meet over q (the partials themselves stay), y
    // goes through sixteen LDS elements (g's place: it is spent) and w = W^H y is one more matrix-vector product in stage 5's
    // form, on four elements of W the lane loads once.  Which lane takes a column does not depend on the rank list, so a rank's
    // filter has the same bits whatever other ranks the launch asks for.
    {
        const int i16 = lane & 15, q4 = lane >> 4;
        T ax = 0, ay = 0;
        int done = q4;
        // W[4 q + ll][i]; a bin whose Cholesky failed has no W (sB holds what the elimination left) and gets zeros
        C wl[4];
#pragma unroll
        for (int ll = 0; ll < 4; ++ll) wl[ll] = (status != 1) ? sB[(4 * q4 + ll) * LD + i16] : mk<T>(0, 0);
        // the span of the bin (gevd_span.h): no slot goes past s_k.  Without a span s_k = N and the loop is the one it was
        const int s_k = span_limit<true, T>(p.span, z1, k, N, p.ranks[p.nV - 1], status != 1, !HOPS || hop == p.span.last_hop, sLam,
                                      scoef, sOrder, lane);
        for (int t = 0; t < p.nV; ++t) {
            const int V = min(p.ranks[t], s_k);
            if (status != 1) {
                for (; done < V; done += 4) {
                    const int c = sOrder[done];
                    const C cf = scoef[c], v = sA[i16 * LD + c];
                    ax = fma_t(-cf.y, v.y, fma_t(cf.x, v.x, ax));
                    ay = fma_t(cf.y, v.x, fma_t(cf.x, v.y, ay));
                }
            }
            if constexpr (sizeof(T) == 8) {
                const T ys = rows_sum2(ax, ay);                             // (copies: the partials stay)
                wsync();                                                    // the rank before has read its y
                if (q4 < 2) reinterpret_cast<T*>(&sr[i16])[q4] = ys;
            } else {
                T yx = ax + __shfl_xor(ax, 16, 64), yy = ay + __shfl_xor(ay, 16, 64);
                yx += __shfl_xor(yx, 32, 64); yy += __shfl_xor(yy, 32, 64);
                wsync();                                                    // the rank before has read its y
                if (q4 == 0) sr[i16] = mk<T>(yx, yy);
            }
            wsync();
            T wx = 0, wy = 0;
#pragma unroll
            for (int ll = 0; ll < 4; ++ll) {
                const C y = sr[4 * q4 + ll];
                wx = fma_t(wl[ll].y, y.y, fma_t(wl[ll].x, y.x, wx));       // conj(W[l][i]) y_l
                wy = fma_t(-wl[ll].y, y.x, fma_t(wl[ll].x, y.y, wy));
            }
            if constexpr (sizeof(T) == 8) {
                // rows 0 and 1 store a part each: the same bytes at the same addresses, from 32 lanes
                const T ws = rows_sum2(wx, wy);
                if (q4 < 2) {
                    const size_t o = 2 * (((size_t)k * p.nV + t) * N + i16) + q4;
                    if (p.out_c128) reinterpret_cast<double*>(pw)[o] = (double)ws;
                    else reinterpret_cast<float*>(pw)[o] = (float)ws;
                }
            } else {
                wx += __shfl_xor(wx, 16, 64); wy += __shfl_xor(wy, 16, 64);
                wx += __shfl_xor(wx, 32, 64); wy += __shfl_xor(wy, 32, 64);
                if (lane < N) {
                    const size_t o = ((size_t)k * p.nV + t) * N + lane;
                    if (p.out_c128) reinterpret_cast<double2*>(pw)[o] = make_double2((double)wx, (double)wy);
                    else reinterpret_cast<float2*>(pw)[o] = make_float2((float)wx, (float)wy);
                }
            }
        }
    }
    if (lane < N) {
        if (plam != nullptr) {
            const T lv = (status != 1) ? sLam[sOrder[lane]] : (T)0;
            if (p.out_c128) reinterpret_cast<double*>(plam)[(size_t)k * N + lane] = (double)lv;
            else reinterpret_cast<float*>(plam)[(size_t)k * N + lane] = (float)lv;
        }
    }
    if (p.U != nullptr) {
        // X = W^H Q, one complex MFMA product, for the caller that asks for the eigenvectors only (the filter above is formed the
        // same way with and without them)
        if (status != 1) {
            C xacc[4];
            cmm16([&](int r, int kx) { const C w = sB[kx * LD + r]; return mk<T>(w.x, -w.y); },
                  [&](int kx, int c) { return sA[kx * LD + c]; }, lane, xacc);
            wsync();
#pragma unroll
            for (int t = 0; t < 4; ++t) sA[mfma_row<T>(lane, t) * LD + (lane & 15)] = xacc[t];
            wsync();
        }
        C* U = reinterpret_cast<C*>(p.U) + (size_t)k * N * N;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int idx = lane + 64 * t, ii = idx >> 4, j = idx & 15;
            U[idx] = (status != 1) ? sA[ii * LD + sOrder[j]] : mk<T>(0, 0);
        }
    }
    if (pstatus != nullptr && lane == 0) pstatus[k] = status;
    stamp(7);
}

// The double kernel is held to four waves per SIMD (its float32 pre-solve and the re-orthonormalisation products would
// otherwise raise the register count past 128 and cost a wave); the float kernel is left to the compiler.
template <typename T, bool FUSED, typename XT, bool DBG = false>
__global__ void __launch_bounds__(64) gevd16m_kernel(const GevdParams p) { gevd16m_body<T, FUSED, XT, DBG>(p, blockIdx.x, blockIdx.y == 1); }
template <bool FUSED, typename XT, bool DBG = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) gevd16m_kernel_f64(const GevdParams p) {
    gevd16m_body<double, FUSED, XT, DBG>(p, blockIdx.x, blockIdx.y == 1);
}
// The float64 streaming front-end's grouped spectra (p.x_group = GS).  Workgroups go to the eight XCDs round robin by their linear
// index and the GS bins of a group read the same lines: index 8 GS q + 8 r + x (x = XCD, r < GS) takes bin 8 GS q + GS x + r, so
// that a group's bins share one L2 (the last, partial block of 8 GS keeps its order).
template <int GS>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) gevd16m_kernel_f64_grouped(const GevdParams p) {
    constexpr int BLK = 8 * GS;
    const int id = blockIdx.x;
    const int k = ((id | (BLK - 1)) < p.K) ? ((id & ~(BLK - 1)) | ((id & 7) * GS) | ((id >> 3) & (GS - 1))) : id;
    gevd16m_body<double, true, double2, false, GS>(p, k, blockIdx.y == 1);
}
// The hops of a chunk in one launch (chunked whole-signal path: blockIdx.z = hop), bin-major (GS = 1) or grouped spectra.  A hop's 2050
// waves are two per SIMD -- all head and tail; sixteen hops are a launch of the headline's size.
template <int GS>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) gevd16m_kernel_f64_hops(const GevdParams p) {
    constexpr int BLK = 8 * GS;
    const int id = blockIdx.x;
    const int k = (GS > 1 && (id | (BLK - 1)) < p.K) ? ((id & ~(BLK - 1)) | ((id & 7) * GS) | ((id >> 3) & (GS - 1))) : id;
    gevd16m_body<double, true, double2, false, GS, true>(p, k, blockIdx.y == 1, blockIdx.z);
}

// the same for c64 slabs (float32 front end): float64 arithmetic ("mixed") and float32 arithmetic
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) gevd16m_kernel_f64_hops_c64(const GevdParams p) {
    gevd16m_body<double, true, float2, false, 1, true>(p, blockIdx.x, blockIdx.y == 1, blockIdx.z);
}
__global__ void __launch_bounds__(64) gevd16m_kernel_f32_hops_c64(const GevdParams p) {
    gevd16m_body<float, true, float2, false, 1, true>(p, blockIdx.x, blockIdx.y == 1, blockIdx.z);
}

}  // namespace

bool apv_gevd16m_takes_hops(const GevdParams& p, int compute_dtype, bool fused) {
    if (!(p.n == 16 && p.reg_mode == APV_REG_ABS && p.reg_bright == 0.0 && fused && p.debug_stop == 0 && p.stamps == nullptr && p.n_hops <= 65535))
        return false;
    if (p.x_c128) return compute_dtype == APV_F64 && (p.x_group <= 1 || p.x_group == 4);
    return p.x_group <= 1;          // c64 slabs: either arithmetic, bin-major
}

hipError_t apv_launch_gevd16m(const GevdParams& p, int compute_dtype, bool fused, hipStream_t s) {
    if (p.n != 16 || p.reg_mode != APV_REG_ABS || p.reg_bright != 0.0) return hipErrorNotSupported;
    if (p.K <= 0) return hipSuccess;
    const dim3 grid(p.K, p.n_zones > 1 ? 2 : 1);
    const bool xd = fused && p.x_c128;
    if (p.n_hops > 1) {
        if (!apv_gevd16m_takes_hops(p, compute_dtype, fused)) return hipErrorInvalidValue;
        const dim3 grid3(p.K, p.n_zones > 1 ? 2 : 1, p.n_hops);
        if (!p.x_c128) {
            if (compute_dtype == APV_F64) hipLaunchKernelGGL(gevd16m_kernel_f64_hops_c64, grid3, dim3(64), 0, s, p);
            else hipLaunchKernelGGL(gevd16m_kernel_f32_hops_c64, grid3, dim3(64), 0, s, p);
            return hipGetLastError();
        }
        if (p.x_group == 4) hipLaunchKernelGGL(gevd16m_kernel_f64_hops<4>, grid3, dim3(64), 0, s, p);
        else hipLaunchKernelGGL(gevd16m_kernel_f64_hops<1>, grid3, dim3(64), 0, s, p);
        return hipGetLastError();
    }
    if (p.x_group > 1) {
        // only the float64 product kernel on c128 slabs reads the grouped layout (apv_gevd16m_reads_groups says when)
        if (!xd || compute_dtype != APV_F64 || p.debug_stop != 0 || p.stamps != nullptr) return hipErrorInvalidValue;
        if (p.x_group == 4) hipLaunchKernelGGL(gevd16m_kernel_f64_grouped<4>, grid, dim3(64), 0, s, p);
        else return hipErrorInvalidValue;
        return hipGetLastError();
    }
    if (p.debug_stop != 0 || p.stamps != nullptr) {
        // diagnostic instantiations (probes only): stage cuts, A/B switches, stage stamps
        if (compute_dtype == APV_F64) {
            if (xd) hipLaunchKernelGGL((gevd16m_kernel_f64<true, double2, true>), grid, dim3(64), 0, s, p);
            else if (fused) hipLaunchKernelGGL((gevd16m_kernel_f64<true, float2, true>), grid, dim3(64), 0, s, p);
            else hipLaunchKernelGGL((gevd16m_kernel_f64<false, float2, true>), grid, dim3(64), 0, s, p);
        } else {
            if (xd) hipLaunchKernelGGL((gevd16m_kernel<float, true, double2, true>), grid, dim3(64), 0, s, p);
            else if (fused) hipLaunchKernelGGL((gevd16m_kernel<float, true, float2, true>), grid, dim3(64), 0, s, p);
            else hipLaunchKernelGGL((gevd16m_kernel<float, false, float2, true>), grid, dim3(64), 0, s, p);
        }
        return hipGetLastError();
    }
    if (compute_dtype == APV_F64) {
        if (xd) hipLaunchKernelGGL((gevd16m_kernel_f64<true, double2>), grid, dim3(64), 0, s, p);
        else if (fused) hipLaunchKernelGGL((gevd16m_kernel_f64<true, float2>), grid, dim3(64), 0, s, p);
        else hipLaunchKernelGGL((gevd16m_kernel_f64<false, float2>), grid, dim3(64), 0, s, p);
    } else {
        if (xd) hipLaunchKernelGGL((gevd16m_kernel<float, true, double2>), grid, dim3(64), 0, s, p);
        else if (fused) hipLaunchKernelGGL((gevd16m_kernel<float, true, float2>), grid, dim3(64), 0, s, p);
        else hipLaunchKernelGGL((gevd16m_kernel<float, false, float2>), grid, dim3(64), 0, s, p);
    }
    return hipGetLastError();
}
