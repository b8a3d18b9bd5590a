// limb_ops.h - the field and point functions one by one on RAW LIMBS, for the tests at the limits of the magnitude contract of fe256.h.
// (host and device: k_diag_limbs in aux_kernels.h and dh_limb_op in csrc/tools/devsrc_host.cpp both call limb_op; the list of operations is
// written here and nowhere else)
//
// Every other test enters through fe_from_words, so its operands are canonical (or small sums of canonical values) and no limb is ever
// near m * 2^29.  Here the nine limbs of each operand go into `fe` as they are and the nine limbs of each result come back as they are:
// nothing is normalised on the way in or out, so a test can put every limb at the ceiling of its documented magnitude and can check the
// documented magnitude of what comes back (tests/limb_cases.py lists the magnitudes beside each operation).
#pragma once
#include "ec.h"
#include "emit33.h"
#include "pub_emit.h"

#define LIMB_IN 6   /* input elements per case */
#define LIMB_OUT 4  /* output elements per case */
enum {
  LIMB_MUL = 0,         // out0 = fe_mul(in0, in1)
  LIMB_SQR = 1,         // out0 = fe_sqr(in0)
  LIMB_MUL2 = 2,        // fe_mul2(out0, out1, in0, in1, in2, in3)
  LIMB_SQR2 = 3,        // fe_sqr2(out0, out1, in0, in1)
  LIMB_WEAK = 4,        // out0 = in0 after fe_normalize_weak
  LIMB_NORM = 5,        // out0 = in0 after fe_normalize; out1.n[0..7] = its 8 words (fe_to_words)
  LIMB_PARITY = 6,      // flag = fe_parity(in0)
  LIMB_IS_ZERO = 7,     // flag = fe_is_zero(in0)
  LIMB_NEG1 = 8,        // out0 = fe_neg(in0, m) for m = 1 .. 6: LIMB_NEG1 + m - 1
  LIMB_NEG6 = 13,
  LIMB_INV_DIVSTEPS = 14,  // out0 = fe_inv_divsteps(in0); out1.n[0..7] = the words of out0 as it stands (it is canonical)
  LIMB_INV_FERMAT = 15,    // out0 = fe_inv_fermat(in0) (magnitude 1); out1.n[0..7] = the words of its canonical residue
  // points.  in: X, Y, ZZ (Jacobian: Z), ZZZ, qx, qy.  out: X3, Y3, ZZ3 (Z3), ZZZ3.  flag: inf of the result
  LIMB_XYZZ_MADD = 16,      // xyzz_madd_lazy(p, qx, qy, 0)
  LIMB_XYZZ_MADD_NEG = 17,  // xyzz_madd_lazy(p, qx, qy, 1)
  LIMB_XYZZ_MMADD = 18,     // xyzz_mmadd_lazy(X, Y, qx, qy)
  LIMB_JAC_MADD = 19,       // jac_madd(p, qx, qy), inputs with h != 0
  LIMB_JAC_MADD_NEG = 20,   // the same function on inputs built with h = 0, rr != 0 (P = -Q: infinity)
  LIMB_JAC_MADD_DBL = 21,   // ... and with h = 0, rr = 0 (P = Q: the doubling)
  LIMB_JAC_DBL = 22,        // jac_dbl(p)
  // public keys by x (pub_emit.h)
  LIMB_PUB_PAIR_X = 23,   // pub_pair_x(out0, out1, X = in0, Y = in1, gx = in2, gy = in3, invk = in4)
  LIMB_PUB_ENDO_X = 24,   // pub_endo_x(out0, out1, in0)
  LIMB_PUB_WORDS20 = 25,  // out0.n[0..4] = pub_words20(in0)
  // the addr33-only emit path of the add kernels (emit33.h), x = in0 (magnitude <= 4), y = in1 (magnitude <= 3)
  LIMB_EMIT33 = 26,       // out0 = the nine SHA-256 message words (prefix byte in place), out1.n[0..4] = the h160_t words of the hash160,
                          // out1.n[5], n[6] = probe 0's index (low, high word) from the native words; flag = emit33_parity(y)
  LIMB_PAR33 = 27,        // flag = emit33_ypar(lam = in0 (magnitude 1), b = in1 (magnitude <= 6), Y = in2 (magnitude 1)): the parity of lam b - Y;
                          // out0.n[0] = 1 when the exact product was taken
  LIMB_OPS = 28
};

// outputs an operation does not produce are zero; returns false for an unknown op (nothing else fails)
FE_FN bool limb_op(int op, const fe in[LIMB_IN], fe out[LIMB_OUT], u32& flag) {
#pragma unroll
  for (int i = 0; i < LIMB_OUT; ++i) out[i] = fe_zero();
  flag = 0;
  switch (op) {
  case LIMB_MUL: out[0] = fe_mul(in[0], in[1]); break;
  case LIMB_SQR: out[0] = fe_sqr(in[0]); break;
  case LIMB_MUL2: fe_mul2(out[0], out[1], in[0], in[1], in[2], in[3]); break;
  case LIMB_SQR2: fe_sqr2(out[0], out[1], in[0], in[1]); break;
  case LIMB_WEAK:
    out[0] = in[0];
    fe_normalize_weak(out[0]);
    break;
  case LIMB_NORM:
    out[0] = in[0];
    fe_normalize(out[0]);
    fe_to_words(out[1].n, out[0]);
    break;
  case LIMB_PARITY: flag = fe_parity(in[0]); break;
  case LIMB_IS_ZERO: flag = fe_is_zero(in[0]) ? 1u : 0u; break;
  case LIMB_NEG1: out[0] = fe_neg(in[0], 1); break;
  case LIMB_NEG1 + 1: out[0] = fe_neg(in[0], 2); break;
  case LIMB_NEG1 + 2: out[0] = fe_neg(in[0], 3); break;
  case LIMB_NEG1 + 3: out[0] = fe_neg(in[0], 4); break;
  case LIMB_NEG1 + 4: out[0] = fe_neg(in[0], 5); break;
  case LIMB_NEG6: out[0] = fe_neg(in[0], 6); break;
  case LIMB_INV_DIVSTEPS:
    out[0] = fe_inv_divsteps(in[0]);
    fe_to_words(out[1].n, out[0]);
    break;
  case LIMB_INV_FERMAT: {
    out[0] = fe_inv_fermat(in[0]);
    fe c = out[0];
    fe_normalize(c);
    fe_to_words(out[1].n, c);
    break;
  }
  case LIMB_XYZZ_MADD:
  case LIMB_XYZZ_MADD_NEG: {
    xyzz p;
    p.X = in[0], p.Y = in[1], p.ZZ = in[2], p.ZZZ = in[3], p.inf = 0;
    const xyzz r = xyzz_madd_lazy(p, in[4], in[5], op == LIMB_XYZZ_MADD_NEG ? 1u : 0u);
    out[0] = r.X, out[1] = r.Y, out[2] = r.ZZ, out[3] = r.ZZZ, flag = r.inf;
    break;
  }
  case LIMB_XYZZ_MMADD: {
    const xyzz r = xyzz_mmadd_lazy(in[0], in[1], in[4], in[5]);
    out[0] = r.X, out[1] = r.Y, out[2] = r.ZZ, out[3] = r.ZZZ, flag = r.inf;
    break;
  }
  case LIMB_JAC_MADD:
  case LIMB_JAC_MADD_NEG:
  case LIMB_JAC_MADD_DBL: {
    jac p;
    p.X = in[0], p.Y = in[1], p.Z = in[2], p.inf = 0;
    const jac r = jac_madd(p, in[4], in[5]);
    out[0] = r.X, out[1] = r.Y, out[2] = r.Z, flag = r.inf;
    break;
  }
  case LIMB_JAC_DBL: {
    jac p;
    p.X = in[0], p.Y = in[1], p.Z = in[2], p.inf = 0;
    const jac r = jac_dbl(p);
    out[0] = r.X, out[1] = r.Y, out[2] = r.Z, flag = r.inf;
    break;
  }
  case LIMB_PUB_PAIR_X: pub_pair_x(out[0], out[1], in[0], in[1], in[2], in[3], in[4]); break;
  case LIMB_PUB_ENDO_X: pub_endo_x(out[0], out[1], in[0]); break;
  case LIMB_PUB_WORDS20: pub_words20(out[0].n, in[0]); break;
  case LIMB_EMIT33: {
    u32 o[5];
    emit33_xwords(out[0].n, in[0]);
    flag = emit33_parity(in[1]);
    out[0].n[0] |= (0x02u | flag) << 24;
    emit33_hash(o, out[0].n);
    emit33_h160(out[1].n, o);
    const u64 idx = emit33_index0(o);
    out[1].n[5] = (u32)idx, out[1].n[6] = (u32)(idx >> 32);
    break;
  }
  case LIMB_PAR33: flag = emit33_ypar(in[0], in[1], in[2], &out[0].n[0]); break;
  default: return false;
  }
  return true;
}
