// mul_check.inc - the body of the `mul` kernel, instantiated twice by mul_kernels.h: as k_mul_check (address types addr33 / addr65)
// and as k_mul_check_p2sh (the same sets plus P2SH, and P2SH alone), like add_walk.inc.  Included with ECL_MUL_KERNEL and ECL_MUL_P2SH
// defined; no include guard on purpose.  With ECL_MUL_ETH defined as well the kernel is k_mul_check_eth: the Ethereum address alone.
// With ECL_MUL_TR defined the kernel is k_mul_points_tr: the Taproot emit kernel, tr_emit in place of check_point, no rings.
// With ECL_MUL_PUB defined the kernel is k_mul_check_pub: public keys by x - Y ZZ is neither formed nor parked (its planes of `tmp` stay
// unused), x = X ZZZ / T alone goes to pub_check.
#if !defined(ECL_MUL_ETH) && !defined(ECL_MUL_TR) && !defined(ECL_MUL_PUB)
template <bool A33, bool A65>
#endif
__global__ void __launch_bounds__(256, ECL_MUL_WAVES) ECL_MUL_KERNEL(const u32* __restrict__ k, u32 n, u32 base, const wtab gtab, add_args a,
                                                      u32* __restrict__ tmp, u32 nt, u32 R) {
#ifdef ECL_MUL_ETH
  constexpr bool A33 = false, A65 = false, ETH = true;
#else
  constexpr bool ETH = false;
#endif
#ifndef ECL_MUL_TR
  constexpr bool P2SH = ECL_MUL_P2SH || ETH;  // (for the rings: the record's type field keeps two bits)
  __shared__ u32 q_mem[4][2][8 * ECL_Q_SLOTS];  // two candidate rings per wave (add_kernel.h)
#endif
  const u32 t = blockIdx.x * 256u + threadIdx.x;
  if (t >= nt) return;  // nt is a multiple of 256: whole workgroups leave
  fe prod = fe_one();
  u32 infmask = 0;
  // parked per scalar: X * ZZZ, Y * ZZ, T = ZZ * ZZZ and the running product of the T's; x = X ZZZ / T, y = Y ZZ / T
#pragma unroll 1
  for (u32 r = 0; r < R; ++r) {
    const u32 i = r * nt + t;
    if (i >= n) break;
    u32 bad;
    xyzz acc = wtab_sum_fast(k + (size_t)i * 8, gtab, bad);
    acc.inf = 0;
    // a zero digit (stand-in point), or P = +-Q on the way (h = 0: only scalars that are 0 (mod n) or built around n) which leaves ZZ = 0 -
    // and a zero in the product chain would take the thread's other scalars with it: the complete sum, out of line
    if (__builtin_expect(bad || fe_is_zero(acc.ZZ), 0)) {
      u32 kk[9];
#pragma unroll
      for (int j = 0; j < 8; ++j) kk[j] = k[(size_t)i * 8 + j];
      kk[8] = 0;
      acc = xyzz_from_jac(wtab_sum_complete(kk, gtab));
    }
    infmask |= (acc.inf ? 1u : 0u) << r;
    fe tt, xs, ys, nprod;
    fe_mul_pair(tt, xs, acc.ZZ, acc.ZZZ, acc.X, acc.ZZZ);
    if (acc.inf) tt = fe_one();
#ifdef ECL_MUL_PUB
    nprod = fe_mul(prod, tt);
#else
    fe_mul_pair(ys, nprod, acc.Y, acc.ZZ, prod, tt);
#endif
    u32* p = tmp + (size_t)r * 36 * nt + t;
#pragma unroll
    for (int l = 0; l < FE_LIMBS; ++l) {
#ifdef ECL_MUL_PUB
      p[(size_t)l * nt] = xs.n[l];
#else
      p[(size_t)l * nt] = xs.n[l], p[(size_t)(9 + l) * nt] = ys.n[l];
#endif
      p[(size_t)(18 + l) * nt] = tt.n[l], p[(size_t)(27 + l) * nt] = prod.n[l];
    }
    prod = nprod;
  }
  fe inv = fe_inv(prod);
  // the filter test through the add kernel's two candidate rings per wave (add_kernel.h: survivors of probe 0 are parked in LDS and
  // finished 64 at a time): every lane of the wave walks all R rounds - a lane without a scalar (i >= n) or with the point at infinity
  // comes along with live = false and leaves the inversion chain alone - so that the rings' wave-uniform state stays uniform
  // (+1.7 % at the .blf design density against finishing every hash's test in place, profiles/r04_mul_rings.txt)
  cand_queues q;
#ifndef ECL_MUL_TR
  q.a.mem = q_mem[threadIdx.x >> 6][0], q.a.head = 0, q.a.count = 0;
  q.b.mem = q_mem[threadIdx.x >> 6][1], q.b.head = 0, q.b.count = 0;
#endif
  q.keys = 0;
#pragma unroll 1
  for (u32 r = R; r-- > 0;) {
    const u32 i = r * nt + t;
    const bool have = i < n;
    const u32* p = tmp + (size_t)r * 36 * nt + t;
    fe X, Y, T, pre;
#pragma unroll
    for (int l = 0; l < FE_LIMBS; ++l) {
#ifdef ECL_MUL_PUB
      X.n[l] = have ? p[(size_t)l * nt] : 0u;
#else
      X.n[l] = have ? p[(size_t)l * nt] : 0u, Y.n[l] = have ? p[(size_t)(9 + l) * nt] : 0u;
#endif
      T.n[l] = have ? p[(size_t)(18 + l) * nt] : (l == 0 ? 1u : 0u), pre.n[l] = have ? p[(size_t)(27 + l) * nt] : 0u;
    }
    fe ti, ninv, x, y;
    fe_mul_pair(ti, ninv, inv, pre, inv, T);  // T = 1 for a lane without a scalar in this round
    inv = ninv;
#ifdef ECL_MUL_PUB
    x = fe_mul(X, ti);
#else
    fe_mul_pair(x, y, X, ti, Y, ti);
#endif
    keys_count(q, have);  // a scalar whose point is at infinity counts: it has nothing to hash
#if defined(ECL_MUL_PUB)
    pub_check<false>(a, q, have && !((infmask >> r) & 1u), x, (u64)base + i);
  }
  cand1_flush<5u, true>(a, q);
#elif defined(ECL_MUL_TR)
    tr_emit(a, have, (infmask >> r) & 1u, x, y, (u64)base + i);  // (base = 0: the piece is its own slab)
  }
#else
    check_point<A33, A65, ECL_MUL_P2SH, false, ETH>(a, &q, have && !((infmask >> r) & 1u), x, y, (u64)base + i);
  }
  cand_flush<P2SH>(a, q);
#endif
  keys_flush(a, q);
}
