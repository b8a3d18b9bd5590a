// add_walk.inc - the body of the add kernel, instantiated twice by add_kernel.h: as k_add (address types addr33 / addr65) and as
// k_add_p2sh (the same sets plus P2SH, and P2SH alone).  Included with ECL_WALK_KERNEL (the kernel's name), ECL_WALK_P2SH and
// ECL_WALK_WAVES (waves per SIMD of an instantiation, an expression of A33 / A65 / ENDO) defined; no include guard on purpose.
// With ECL_WALK_ETH defined as well the kernel is k_add_eth<ENDO>: the Ethereum address alone (ECL_WALK_WAVES an expression of ENDO).
// With ECL_WALK_TR defined the kernel is k_add_tr (no template): the Taproot emit kernel, tr_emit in place of check_point, no rings.
// With ECL_WALK_PUB defined the kernel is k_add_pub<ENDO>: public keys by x - no y of a walked point, pub_check in place of check_point.
// With ECL_WALK_PREFIX defined (alone or beside ECL_WALK_ETH) the kernel is k_add_pfx<A33, A65, ENDO> / k_add_pfx_eth<ENDO>: the prefix
// filter (prefix.h) in place of the bloom, one candidate ring.
// With ECL_WALK_MASK defined beside ECL_WALK_PREFIX and ECL_WALK_ETH the kernel is k_add_msk_eth<ENDO>: the mask filter (mask.h) in place of
// the prefix filter, the same one ring.
// With ECL_WALK_INSERT defined beside ECL_WALK_PUB the kernel is k_add_pub_ins (no template): pub_insert in place of pub_check, no rings.
#if defined(ECL_WALK_TR) || defined(ECL_WALK_INSERT)
#elif defined(ECL_WALK_ETH) || defined(ECL_WALK_PUB)
template <bool ENDO>
#else
template <bool A33, bool A65, bool ENDO>
#endif
__global__ void __launch_bounds__(ECL_ADD_BLOCK, ECL_WALK_WAVES) ECL_WALK_KERNEL(const add_args a) {
#if defined(ECL_WALK_ETH)
  constexpr bool A33 = false, A65 = false, ETH = true;
#else
  constexpr bool ETH = false;
#endif
  // the addr33-only kernels (k_add<true, false, ENDO>) take y's parity from a partial product and never form y of a walked point (emit33.h)
#if defined(ECL_WALK_TR) || defined(ECL_WALK_INSERT) || defined(ECL_WALK_PUB) || defined(ECL_WALK_PREFIX)
  constexpr bool PAR33 = false, PAR33_CALL = false;
#else
  constexpr bool PAR33 = A33 && !A65 && !ECL_WALK_P2SH && !ETH, PAR33_CALL = PAR33 && !ENDO;  // (the exact way: out of line / in place)
#endif
#if defined(ECL_WALK_TR) || defined(ECL_WALK_INSERT)
  cand_queues q;  // (the key count alone)
  q.keys = 0;
#else
  constexpr bool P2SH = ECL_WALK_P2SH || ETH;  // (for the rings: the record's type field keeps two bits)
#if defined(ECL_WALK_PREFIX)
  __shared__ u32 q_mem[ECL_ADD_BLOCK / 64][1][8 * ECL_Q_SLOTS];  // one candidate ring per wave
  cand_queues q;
  q.a.mem = q_mem[threadIdx.x >> 6][0], q.a.head = 0, q.a.count = 0;
  q.b.mem = nullptr, q.b.head = 0, q.b.count = 0;
#else
  __shared__ u32 q_mem[ECL_ADD_BLOCK / 64][2][8 * ECL_Q_SLOTS];  // two candidate rings per wave
  cand_queues q;
  q.a.mem = q_mem[threadIdx.x >> 6][0], q.a.head = 0, q.a.count = 0;
  q.b.mem = q_mem[threadIdx.x >> 6][1], q.b.head = 0, q.b.count = 0;
#endif
  q.keys = 0;
#endif
  const u32 g = blockIdx.x * (u32)ECL_ADD_BLOCK + threadIdx.x;
  const u32 T = a.T, B = a.B;
  if (g >= T) return;  // (never taken: T is a multiple of the block size)
  const size_t plane = T;
  // centre (X, Y): canonical in HBM, magnitude 1 in registers
  fe X = fe_ld_words2(a.cxy + g, plane), Y = fe_ld_words2(a.cxy + 2 * (size_t)T + g, plane);
  const fe Jx = fe_ldw(a.jump), Jy = fe_ldw(a.jump + 8);
  const ctab_ptr tab = (ctab_ptr)(uintptr_t)a.tab;
  uint4* scr4 = a.scratch + g;
  u32* scr2 = a.scratch2 + g;
  const size_t s4 = 2 * (size_t)T;  // one chain element = two uint4 planes + one u32 plane

#pragma unroll 1
  for (u32 b = 0; b < a.nb; ++b) {
    const u64 base = ((u64)b * T + g) * (2ull * B);
    // groups only grow: a wave leaves when none of its lanes has keys left (wave-uniform control flow keeps the
    // candidate queue state uniform; the lane count is sized to the range, so idle lanes are rare)
    if (__builtin_amdgcn_ballot_w64(base < a.nkeys) == 0) break;

    // ---- phase 1: prefix products of e_0 = Jx - X, e_k = Gx_{k-1} - X   (differences have magnitude 3)
    fe acc = fe_sub(Jx, X);
    fe_normalize_weak(acc);            // magnitude 1: the chain multiplies it by a magnitude-3 difference
    const bool dbl = fe_is_zero(acc);  // C == J: next centre is 2C (C == -J would be the scalar 0: excluded)
    if (dbl) acc = fe_one();
#pragma unroll 1
    for (u32 k = 1; k <= B; ++k) {
      fe_st_limbs(scr4 + (size_t)(k - 1) * s4, plane, scr2 + (size_t)(k - 1) * plane, acc);
      fe dx = fe_sub(fe_ld_tab(tab + (size_t)(k - 1) * ECL_TAB_STRIDE), X);
      acc = fe_mul(acc, dx);
    }
    // ---- phase 2: one inversion for the whole chain
    fe inv = fe_inv(acc);
    // ---- phase 3: walk the chain backwards, emit C +- G_i.  Each prefix product is loaded at use: loading it one
    // iteration ahead measured 2.9 % slower (profiles/r03_pmc_filter_compare.txt section 4)
#pragma unroll 1
    for (u32 k = B; k >= 1; --k) {
      const u32 i = k - 1;
      const fe pre = fe_ld_limbs(scr4 + (size_t)i * s4, plane, scr2 + (size_t)i * plane);
      const fe gx = fe_ld_tab(tab + (size_t)i * ECL_TAB_STRIDE), gy = fe_ld_tab(tab + (size_t)i * ECL_TAB_STRIDE + FE_LIMBS);
      const fe dx = fe_sub(gx, X);
      const fe invk = fe_mul(inv, pre);  // 1 / (Gx_i - X)
      inv = fe_mul(inv, dx);
      const fe nxg = fe_neg(fe_add(X, gx), 2);  // -(X + Gx), magnitude 3
      const int nwhich = (k == 1) ? 3 : 2;
#pragma unroll 1
      for (int which = 0; which < nwhich; ++which) {
        fe px, py;
        u32 par = 0;  // (PAR33 only)
        u64 off;
        bool valid = true;  // wave-uniform
        if (which < 2) {
          // lambda = (+-Gy - Y) / (Gx - X); x3 = lambda^2 - X - Gx; y3 = lambda (X - x3) - Y   (main.c:379-386)
          // +-Gy - Y, magnitude 3.  The table side (Gy + 2p or 3p - Gy) is wave-uniform like `which`: selected on
          // the scalar unit, so the vector side is one subtraction per limb (written as a select of two vector
          // results the compiler emits both and nine v_cndmask)
#ifdef ECL_WALK_PUB
          px = pub_x(pub_num(gy, Y, which), invk, nxg);  // magnitude 4; no y (pub_emit.h: the same numerator, the code the host test runs)
#else
          const fe c = which == 0 ? fe_add(gy, fe_neg(fe_zero(), 1)) : fe_neg(gy, 2);
          fe s;
#pragma unroll
          for (int l = 0; l < FE_LIMBS; ++l) s.n[l] = c.n[l] - Y.n[l];
          fe lam = fe_mul(s, invk);
          px = fe_add(fe_sqr(lam), nxg);                                   // magnitude 4
          if constexpr (PAR33) {
            // y3 for its parity alone.  Where the short product may not be relied on (2^-16 per key) the point is walked again from what
            // the loop keeps anyway (add_kernel.h, walk_ypar_exact).  Without the endomorphism out of line.  With it in place - there the
            // call costs two spilled pointers in the table loop; the numerator is formed from an opaque copy of Y, or the compiler shares
            // lam and X - px with the lines above and keeps both across the short product.  Either way the step is walk_ypar_step
            u32 rare;
            par = emit33_ypar_short(lam, fe_add(X, fe_neg(px, 4)), Y, rare);
            if (__builtin_expect(rare != 0, 0)) {
              if constexpr (!PAR33_CALL) {
                fe Yh = Y;
#pragma unroll
                for (int l = 0; l < FE_LIMBS; ++l) {
                  FE_HIDE24(Yh.n[l]);
                  s.n[l] = c.n[l] - Yh.n[l];
                }
                par = walk_ypar_step(px, s, invk, nxg, X, Y);  // (px again: the same value, and the first one need not be kept)
              } else {
                const fe Xc = walk_ypar_copy(X), Yc = walk_ypar_copy(Y), invkc = walk_ypar_copy(invk);
                par = walk_ypar_exact(tab + (size_t)i * ECL_TAB_STRIDE, which, Xc, Yc, invkc);
              }
            }
          } else {
            py = fe_sub(fe_mul(lam, fe_add(X, fe_neg(px, 4))), Y);         // X - px: magnitude 6; py: magnitude 3
          }
#endif
          off = base + (which == 0 ? B + 1 + i : B - 1 - i);  // scalar select, one 64-bit add
          valid = which == 1 || i + 1 < B;
        } else {
#ifdef ECL_WALK_PUB
          px = X, off = base + B;
#pragma unroll
          for (int l = 0; l < FE_LIMBS; ++l) FE_HIDE24(px.n[l]);
        }
#else
          px = X, py = Y, off = base + B;
          // the centre itself, once per B iterations: keep the copies of X and Y inside this branch (left alone, the
          // compiler copies them into px / py at the head of EVERY iteration and overwrites them: 18 moves per key)
#pragma unroll
          for (int l = 0; l < FE_LIMBS; ++l) {
            FE_HIDE24(px.n[l]);
            FE_HIDE24(py.n[l]);
          }
          if constexpr (PAR33) par = emit33_parity(py);
        }
#endif
        if (valid) {
          const bool live = off < a.nkeys;
          keys_count(q, live);
#if defined(ECL_WALK_TR)
          tr_emit(a, live, false, px, py, off);
#elif defined(ECL_WALK_INSERT)
          pub_insert(a, live, px);
#elif defined(ECL_WALK_PUB)
          pub_check<ENDO>(a, q, live, px, off);
#elif defined(ECL_WALK_MASK)
          check_point<A33, A65, false, ENDO, ETH, 2>(a, &q, live, px, py, off);
#elif defined(ECL_WALK_PREFIX)
          check_point<A33, A65, false, ENDO, ETH, 1>(a, &q, live, px, py, off);
#else
          if constexpr (PAR33) check_point33<ENDO>(a, &q, live, px, par, off);
          else check_point<A33, A65, ECL_WALK_P2SH, ENDO, ETH>(a, &q, live, px, py, off);
#endif
        }
      }
    }
    // ---- next centre: C + J with 1/(Jx - X) = inv (or the tangent if C == J)
    fe lam;
    if (!dbl) {
      lam = fe_mul(fe_sub(Jy, Y), inv);
    } else {
      fe x2 = fe_sqr(X);
      lam = fe_mul(fe_add(fe_add(x2, x2), x2), fe_inv(fe_add(Y, Y)));
    }
    fe Xn = fe_add(fe_sqr(lam), fe_neg(fe_add(X, Jx), 2));           // magnitude 4
    fe Yn = fe_sub(fe_mul(lam, fe_add(X, fe_neg(Xn, 4))), Y);        // magnitude 3
    fe_normalize_weak(Xn);
    fe_normalize_weak(Yn);
    X = Xn, Y = Yn;
  }
#if defined(ECL_WALK_INSERT)
#elif defined(ECL_WALK_PUB)
  cand1_flush<5u, true>(a, q);
#elif defined(ECL_WALK_MASK)
  mask_flush(a, q);
#elif defined(ECL_WALK_PREFIX)
  prefix_flush(a, q);
#elif !defined(ECL_WALK_TR)
  cand_flush<P2SH>(a, q);
#endif
  keys_flush(a, q);
  fe_st_words2(a.cxy + g, plane, X);
  fe_st_words2(a.cxy + 2 * (size_t)T + g, plane, Y);
}
