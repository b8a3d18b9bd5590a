/*
 * ecloop_hip.h — C ABI of the MI355X (gfx950) key-search engine: the drop-in boundary for ecloop's hot path.
 *
 * The reference (vladkens/ecloop v0.5.0) has no plugin/FFI seam: the hot path is reached by static calls inside
 * one translation unit.  This header cuts the seam at the L4 -> L3 call:
 *
 *   reference call site                                   replaced by
 *   ---------------------------------------------------   ------------------------------------------
 *   batch_add(ctx, pk, iterations)          main.c:349    ecl_hip_add_range()
 *     + check_found_add / check_hash        main.c:278-347  (device: hash160 + bloom probe; hits returned)
 *   ctx_precompute_gpoints(ctx)             main.c:219    done inside ecl_hip_open()/first add_range
 *   ec_gtable_init, ec_gtable_mul xN        ecc.c:876-929
 *     + ec_jacobi_grprdc + check_found_mul  main.c:531-534  ecl_hip_mul_batch()  (window tables built on the device)
 *   SHA-256 of each line under -raw         main.c:505-527  ecl_hip_mul_batch_raw()  (hashed on the device)
 *   qsort + blf_add loop of load_filter     main.c:112-131  optional: ecl_hip_sort_list() + ecl_hip_bloom_insert()
 *   blf_has(&ctx->blf, h)                   utils.c:308   device probe of the bits given to ecl_hip_set_bloom()
 *   bsearch(to_find_hashes) in ctx_check_hash main.c:212-216  optional: ecl_hip_set_list() (else on the host, as before)
 *   ctx->check_addr33/65, use_endo, ord_offs main.c:32-34,67  flags / ord_offs of ecl_hip_open()
 *
 * What stays on the host, unchanged in meaning: filter loading (main.c:71-131), the sorted-list confirm after a
 * bloom hit (main.c:212-216), calc_priv (main.c:267-276), pk_verify_hash (main.c:248-263), the found sink and
 * status line (main.c:134-203), the job scheduler (main.c:405-454).  The device reports bloom hits as
 * {key offset, endo index, address type, hash160}; the host turns them into private keys.
 *
 * Plain C types only: pointers, sizes, fixed-width integers.  No stdout/stderr/exit inside the library.
 *
 * Threads.  One handle = one context on one GPU; a handle must be used by ONE host thread at a time (any thread, not two at once);
 * different handles - on the same GPU or on different ones - may be used concurrently without any locking by the caller: one thread
 * per context is the intended pattern (the keyspace is range-partitioned, there is no collective).  What contexts of a process share
 * is guarded inside the library: the window table of `mul` (one per device and width: built once under a mutex by the first context
 * that needs it, read-only from then on, reference-counted, freed with the last context that holds it; a context that switches width
 * waits for its own kernels on both of its streams first), the once-per-process self-test record, and the look-ahead groups of
 * section 3 (sweeps and their records belong to the group of contexts that share a filter; one mutex per group; records are immutable
 * once published).  ecl_hip_strerror returns static text; ecl_hip_last_error returns the handle's own buffer (same thread rule).
 *
 * Exports: exactly the 45 ecl_hip_* functions declared below (the library is linked with a version script; `nm -D` shows nothing else).
 */
#ifndef ECLOOP_HIP_H
#define ECLOOP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the functions declared here are exported */
#pragma GCC visibility push(default)

typedef struct ecl_hip ecl_hip; /* opaque per-device context */

/* flags of ecl_hip_open: which encodings to hash (main.c:819-827) and the endomorphism switch (main.c:829).  ECL_P2SH has no reference
   counterpart: the nested-SegWit (BIP49, P2SH-P2WPKH "3..." address) hash, hash160(0x00 0x14 || hash160 of the compressed key).
   Any non-empty set of the three address types, with or without ECL_ENDO; every other bit is refused (ECL_E_ARG).  The bit 8 is not
   used: releases before ECL_P2SH refused it as an unknown flag, and it stays refused, so ECL_P2SH is the next one.
   ECL_ETH (no reference counterpart either): the Ethereum address, the last 20 bytes of Keccak-256 (original padding) over the 64 bytes
   x || y of the uncompressed key.  Eth is searched ALONE: ECL_ETH together with ECL_ADDR33, ECL_ADDR65 or ECL_P2SH is ECL_E_ARG (a Bitcoin
   list and an Ethereum list are different files), with or without ECL_ENDO.  So the valid type sets are: any non-empty subset of the three
   Bitcoin types, or ECL_ETH by itself.  (ecl_hip_open leaves no handle to ask after ECL_E_ARG - this comment is the message.)  The bits 8
   and 32 stay refused as unknown flags.
   ECL_TR (no reference counterpart): Taproot, the BIP341 / BIP86 key-path output ("bc1p..." addresses) of the key with no script tree.  Its
   output key is not a hash of the public key P but the x of a second point, Q = P' + t G with P' the even-y lift of P and
   t = SHA-256(T || T || P.x), T = SHA-256("TapTweak"); a key with t >= n has no output (probability 2^-128: it counts as covered and is
   not probed).  Filters, lists and records keep their 20-byte entries: a Taproot entry is the LEADING 20 BYTES of the 32-byte output key
   (160 bits, the strength every other type is matched at); the caller verifies a hit with ecl_hip_verify_tr, which gives all 32.  k and
   n - k have the same output key; the key reported is the one that was walked.  Taproot is searched alone and without the endomorphism:
   ECL_TR together with any of ECL_ADDR33, ECL_ADDR65, ECL_P2SH, ECL_ETH or ECL_ENDO is ECL_E_ARG (a Taproot list is a different file;
   the endomorphism amortises the walk, which is a few per cent of a Taproot key, and its (x, -y) images have the same output key).
   A Taproot key costs one fixed-base scalar multiplication, about what a `mul` scalar costs: ecl_hip_add_range walks a call in slabs
   (2^26 keys: the points and tweaks of a slab are parked in 6.4 GB of HBM, then multiplied on the `mul` table of the context;
   environment ECL_HIP_TR_SLAB_LOG2 = 12 ... 28 changes the slab, not the results), and tweaked keys count as scalars for the width
   of that table.
   ECL_PUB (no reference counterpart): the public key itself, matched by its x coordinate - lists of P2PK outputs, spent-from keys, puzzle
   keys with a revealed public key.  Nothing is hashed on the device: the walk emits x alone (no y of a walked point) and the entry of
   filters, lists and records is the LEADING 20 BYTES of x, 160 bits like every other type (the Taproot convention; no new format).  A key
   and its negative share x: the key reported is the one that was walked, the caller re-derives a hit with ecl_hip_diag_mulg (the
   double-and-add kernel: neither the walk nor the window sum; it returns x and y), compares its leading 20 bytes with the record - all a
   record or a list entry holds - and has the whole key from it (all 32 bytes of x, and y for the prefix byte).  With ECL_ENDO a key gives
   three records (x, beta x, beta^2 x: endo = 0, 2, 4), which stand for six keys.  Public keys are searched alone: ECL_PUB is valid by
   itself or with ECL_ENDO; together with any of ECL_ADDR33, ECL_ADDR65, ECL_P2SH, ECL_ETH, ECL_TR (or the refused bits 8 and 32) it is
   ECL_E_ARG.
   ECL_ORIGIN and ECL_INSERT (no reference counterpart): the two walks of a baby-step giant-step search for the key of a KNOWN public key
   (the `bsgs` command; ecloop_amd/host/bsgs_plan.h has the method).  Each is valid in exactly one combination - ECL_PUB | ECL_ORIGIN,
   ECL_PUB | ECL_INSERT - and ECL_E_ARG with ECL_ENDO, with any other type, with each other or without ECL_PUB (but for ECL_ORIGIN beside
   ECL_PREFIX, the split-key search: see ECL_PREFIX).  Neither takes part in
   the look-ahead, and ecl_hip_mul_batch(_raw) on them is ECL_E_ARG.
   ECL_PUB | ECL_ORIGIN: a public-key walk that starts from a point nobody knows the scalar of.  The `start` argument of ecl_hip_add_range
   points to TWELVE limbs: the scalar, then the affine x and y of an origin point O (little-endian u64 limbs, both below p, y^2 = x^3 + 7:
   checked on the host, ECL_E_ARG otherwise), and the call walks the points O + (start + j 2^ord_offs) G, j < nkeys - records, key_offset
   and coverage as for ECL_PUB, the ECL_E_RANGE check on the scalar part as it is (so the caller keeps O + k G finite: a base point that is
   -O makes the call ECL_E_RANGE, any other meeting of the two leaves x values of one group that are no point's - nothing else).  A call
   continues the resident walk only if its origin is the one before's, too.
   ECL_PUB | ECL_INSERT: a public-key walk that SETS the 20 filter bits (blf_add) of the leading 20 bytes of x of every key of the call
   - and of no other point the walk computes - in the resident filter instead of probing them: *nout = 0, keys are counted and the
   coverage check applies; ecl_hip_get_bloom reads the filter back.
   ECL_HERD (no reference counterpart): the herd of a Pollard lambda (kangaroo) search for the key of a KNOWN public key (the `kangaroo`
   command; ecloop_amd/host/kangaroo_plan.h is the definition of the method).  Valid only as ECL_PUB | ECL_HERD: with ECL_ENDO, ECL_ORIGIN,
   ECL_INSERT, any address type or without ECL_PUB it is ECL_E_ARG.  For such a context ord_offs of ecl_hip_open is the number of
   distinguished-point bits dp, 0 ... 32 (more: ECL_E_ARG); no filter is needed (ecl_hip_add_range before ecl_hip_set_bloom is not
   ECL_E_NOBLOOM); it does not take part in the look-ahead, ecl_hip_set_geometry has no effect on it and ecl_hip_mul_batch(_raw) is
   ECL_E_ARG.  The `start` argument of ecl_hip_add_range points to SIXTEEN limbs, the herd's parameter block:
     limbs 0..3    the base scalar B
     limbs 4..11   the affine x and y of the target Q (both below p, y^2 = x^3 + 7: checked on the host, ECL_E_ARG otherwise)
     limb 12       seed
     limb 13       herd_log2, 1 ... 24: H = 2^herd_log2 kangaroos, an even index is tame, an odd one wild
     limb 14       jump_bits jb, 4 ... 120 (32 different distances need 2^(jb + 1) >= 32)
     limb 15       spread_bits sb, 1 ... 124   (any of the three out of its range: ECL_E_ARG)
   and nkeys is the number of JUMPS of the call, a multiple of H (else ECL_E_ARG): every kangaroo makes nkeys / H of them.  A call whose
   sixteen limbs equal the previous call's continues the resident herd; anything else builds the herd anew, which counts as one set-up in
   ecl_hip_get_setup_timing.  The kernel counts the jumps it makes: a call whose count differs from nkeys returns ECL_E_COVERAGE (and
   ecl_hip_diag_drop_round makes that happen), and the next call builds the herd anew.
   The method: the 32 jump distances s_j are drawn from a SplitMix64 stream of seed, 128 bits from two outputs each, s_j = 1 + (v mod
   2^(jb + 1)), a draw equal to an earlier one drawn again; table point T_j = s_j G.  The start offsets r_i = v mod 2^sb follow from the same
   stream.  Tame i starts at (B + r_i) G, wild i at Q + r_i G (the complete addition), both with distance r_i; a start that is the point at
   infinity is ECL_E_RANGE.  A jump: with x canonical, j = bits 32..36 of x, P <- P + T_j, d <- d + s_j; where x(P) = x(T_j) - the sum would be
   a doubling or the point at infinity - the kangaroo takes j + 1 mod 32 for this jump, so the shared inversion never sees a zero.  After
   the jump the point is distinguished if the low dp bits of x are zero, and is reported as one ecl_found record with compressed = 6
   (label dp): endo = 0 tame / 1 wild, key_offset = distance bits 0..63, h160[0], h160[1] = distance bits 96..127 and 64..95, h160[2..4] =
   the leading 12 bytes of x in the h160_t word convention.  Distances are 128-bit: one that would pass 2^128 fails the call with
   ECL_E_RANGE.  ECL_E_OVERFLOW and ecl_hip_fetch_found as for every other context; the order of a call's records is not defined.
   ECL_PREFIX (no reference counterpart): the prefix filter, for addresses that START with given characters (the `-p` option;
   ecloop_amd/host/prefix_plan.h turns patterns into ranges).  In place of a bloom filter the context holds a table of n inclusive ranges
   [lo, hi] over the 160-bit value, words in the record's order (h160[0] most significant), and reports a key iff a hash of it lies inside
   a range: no false positives, no duplicates.  Valid beside ECL_ADDR33 / ECL_ADDR65 with or without ECL_ENDO, or beside ECL_ETH with or
   without ECL_ENDO; with ECL_P2SH, ECL_TR, ECL_PUB, ECL_INSERT or ECL_HERD it is ECL_E_ARG (ECL_ORIGIN: below).  On such a context
     ecl_hip_set_bloom(h, words, nwords) takes the TABLE: nwords = 5 n, each range ten uint32 - lo[5], hi[5] - with 1 <= n <= 65536, lo <= hi,
       the ranges sorted by lo and disjoint; nwords no multiple of 5, n out of range, lo > hi, an unsorted table or overlapping ranges are
       ECL_E_ARG.  The library builds the stage-1 bitmap (one bit per 2^-24 of the space) itself;
     ecl_hip_add_range is ECL_E_NOBLOOM before a table is set and otherwise behaves as always (cap, ECL_E_OVERFLOW, ecl_hip_fetch_found,
       the coverage check); the context never takes part in the look-ahead;
     ecl_hip_set_list, ecl_hip_bloom_insert, ecl_hip_bloom_insert_count, ecl_hip_get_bloom, ecl_hip_mul_batch and ecl_hip_mul_batch_raw are
       ECL_E_ARG;
     ecl_hip_diag_bloom runs the device's two-stage prefix test on the given values (hit = the value lies inside a range).
   ECL_PREFIX | ECL_ORIGIN (the split-key vanity search, `-p` with `-k`): the one hashing combination ECL_ORIGIN is valid in - beside
   ECL_PREFIX and ECL_ADDR33, ECL_ADDR65, both, or ECL_ETH, with or without ECL_ENDO; ECL_ORIGIN on a hashing context without ECL_PREFIX,
   and ECL_PREFIX | ECL_PUB | ECL_ORIGIN, stay ECL_E_ARG.  The context is the prefix context above whose walk starts from the caller's
   point: `start` of ecl_hip_add_range points to TWELVE limbs, treated exactly as ECL_PUB | ECL_ORIGIN treats them (the origin checked on
   the host, ECL_E_ARG; a base point that is -O: ECL_E_RANGE; a call continues the resident walk only if its origin is the one before's;
   no look-ahead; ecl_hip_mul_batch(_raw) ECL_E_ARG), and the call reports the keys j whose point O + (start + j 2^ord_offs) G has a hash
   inside a range - records, key_offset (from the call's scalar), endo (the six images of that point) and compressed as on the plain
   prefix context.  The scalars say nothing about the points' keys: whoever knows the origin's key k_O adds it (host/splitkey.h).  On such
   a context each entry of `k` of ecl_hip_verify / ecl_hip_verify_eth is TWELVE limbs, too - see there.
   ECL_MASK (no reference counterpart): the mask filter, for Ethereum addresses with fixed digits anywhere - a suffix, both ends, holes
   (`-p 0xdead*beef`; ecloop_amd/host/mask_plan.h turns patterns into entries).  In place of a bloom filter the context holds a table of n
   entries, each a mask m and a value v over the 160-bit address, words in the record's order (h160[0] most significant), and reports a
   key iff some entry has (address ^ v) & m == 0: exact, and one record per key and image however many entries match.  Valid only as
   ECL_ETH | ECL_MASK, with or without ECL_ENDO and / or ECL_ORIGIN; beside ECL_PREFIX, ECL_ADDR33, ECL_ADDR65, ECL_P2SH, ECL_TR, ECL_PUB,
   ECL_INSERT or ECL_HERD, or without ECL_ETH, it is ECL_E_ARG.  On such a context
     ecl_hip_set_bloom(h, words, nwords) takes the TABLE: nwords = 5 n, each entry ten uint32 - m[5], v[5] - with 1 <= n <= 16, no bit of
       v outside m and no two identical entries; anything else is ECL_E_ARG and leaves the context without a table.  An all-zero mask is
       legal and matches every address: how much of the space a table may cover is the caller's business (the planner bounds it);
     ecl_hip_add_range, ecl_hip_set_list, ecl_hip_bloom_insert(_count), ecl_hip_get_bloom and ecl_hip_mul_batch(_raw) behave as on a prefix
       context (ECL_E_NOBLOOM before a table is set; the others ECL_E_ARG; no look-ahead);
     ecl_hip_diag_bloom runs the device's mask test on the given values.
   ECL_MASK | ECL_ORIGIN is the split-key search of such patterns and behaves as ECL_PREFIX | ECL_ORIGIN beside ECL_ETH does: twelve limbs
   per `start` and per entry of ecl_hip_verify_eth.
   ECL_KDF_KECCAK, ECL_KDF_SHA3, ECL_KDF_CAMP2 (no reference counterpart): the key derivation function of ecl_hip_mul_batch_raw, a two-bit
   field - none of them: SHA-256 of the line, the Bitcoin brain-wallet convention and the reference's `-raw`.  Ethereum brain wallets
   hash otherwise, and with these bits the device does: the digest of the line's bytes m, read as a big-endian 256-bit number, is
     ECL_KDF_KECCAK  Keccak-256(m): rate 136, capacity 512, first pad byte 0x01, last pad byte 0x80 (old ethaddress, early ethercamp);
     ECL_KDF_SHA3    SHA3-256(m): the same sponge with the first pad byte 0x06 (FIPS 202);
     ECL_KDF_CAMP2   (both bits) d_1 = Keccak-256(m), d_(i+1) = Keccak-256(the 32 bytes of d_i), the digest is d_2031: 2031 hashes in all
                     (the later ethercamp wallet; brainflayer's `camp2`).
   (A length = 135 mod 136 puts both pad bytes into one, 0x81 / 0x86; a length = 0 mod 136 adds a block of padding.)  Valid beside every
   context that has a `mul` - any set of ECL_ADDR33, ECL_ADDR65, ECL_P2SH; ECL_ETH; ECL_TR; ECL_PUB; with ECL_ENDO wherever that context
   allows it - and ECL_E_ARG beside ECL_ORIGIN, ECL_INSERT, ECL_HERD, ECL_PREFIX or ECL_MASK.  ONLY ecl_hip_mul_batch_raw changes: it hashes
   the lines with the chosen function where it hashes them with SHA-256, everything around that (pieces, the text sent along, the repeat
   pass, coverage, overflow, ecl_hip_fetch_found) as it is; ecl_hip_add_range, ecl_hip_mul_batch and every other call behave as on the
   same context without the bits.  ecl_hip_selftest of such a context also runs its hash on known answers (ECL_E_SELFTEST).
   ECL_KDF_BIP39 (no reference counterpart): the lines of ecl_hip_mul_batch_raw are BIP39 phrases and the scalar of a line is a BIP32
   private key of its seed.  Valid beside the contexts the ECL_KDF_* field is valid beside; ECL_E_ARG together with any ECL_KDF_* bit and
   beside ECL_ORIGIN, ECL_INSERT, ECL_HERD, ECL_PREFIX or ECL_MASK.  ONLY ecl_hip_mul_batch_raw changes.  Its parameters travel in band:
   lines[0] of EVERY call is not a phrase but the derivation record, lines[1 .. n - 1] are the phrases, key_offset of a hit is the phrase
   index (lines[1] is phrase 0), and the call asks for n - 1 scalars (coverage counts against that).  The record, packed, little-endian:
       u8 magic[4] = "B39\0";  u8 reuse;  u8 depth (0 .. 10);  u8 pass_len (0 .. 99);  u8 zero;
       u32 path[depth]   (bit 31 = hardened);   u8 pass[pass_len]
   A line length other than 8 + 4 depth + pass_len, a wrong magic, depth > 10, pass_len > 99, a reuse byte other than 0 or 1, a zero byte
   that is not zero, a record or a phrase that lies outside the text, or more than 2^22 phrases are ECL_E_ARG with a message in
   ecl_hip_last_error, and nothing is launched; n = 1 (the record alone) is ECL_OK with no records.  For the phrase bytes m,
   taken as given (no NFKD, no word list, no checksum test):
       seed = PBKDF2-HMAC-SHA512(m, "mnemonic" || pass, 2048 iterations, 64 bytes);  (k, c) = HMAC-SHA512("Bitcoin seed", seed);
       per path element i, CKDpriv: I = HMAC-SHA512(c, 0x00 || ser256(k) || ser32(i)) if hardened, else of serP(k G) || ser32(i);
       k <- I_L + k mod n, c <- I_R;  the scalar is the last k (depth 0: the master key).
   A node BIP32 calls invalid (master I_L = 0 or >= n, a child's I_L >= n, a child key 0) gives the scalar 0, which is counted and not
   probed.  reuse = 0: the phrases are hashed and every phrase's master node (64 bytes) is kept by the context.  reuse = 1: the phrases
   are taken to be those of the call before and are not read; the path is walked from the kept nodes - another index or path costs a few
   HMACs per phrase, not 4096 compressions.  reuse = 1 is ECL_E_ARG when no nodes are kept, when n or pass differs from the kept nodes',
   or when the previous ecl_hip_mul_batch_raw call on the context returned neither ECL_OK nor ECL_E_OVERFLOW (calls of other functions in
   between are not looked at: none of them touches the kept nodes).  ecl_hip_selftest of such a context also runs
   both derivation kernels on BIP39's test phrase (ECL_E_SELFTEST).
   ECL_GEN (no reference counterpart): the lines of ecl_hip_mul_batch_raw are not sent but generated on the device, from a template - masks,
   dictionaries, their combinations (the `brain` command).  Valid beside the contexts the ECL_KDF_* field is valid beside, with or
   without ECL_KDF_KECCAK / ECL_KDF_SHA3 / ECL_KDF_CAMP2; ECL_E_ARG beside ECL_KDF_BIP39, ECL_ORIGIN, ECL_INSERT, ECL_HERD, ECL_PREFIX or
   ECL_MASK, alone, or beside a type set that is itself refused.  ONLY ecl_hip_mul_batch_raw changes: `text` / `text_bytes` are the
   template, `lines` points to ONE u64, the index of the call's first candidate, n (<= 2^26) is the number of candidates, and key_offset
   of a record is index - first.  The template (host/gen_plan.h is its definition): P positions, 1 <= P <= 16; position p has c_p >= 1
   alternatives of 0 ... 255 bytes each; L = the sum over the positions of the longest alternative, at most 256; at most 2^22
   alternatives and 2^28 bytes of them in all; T = the product of the c_p, below 2^64.  Candidate i, 0 <= i < T, has the digits d_p with
   i = sum d_p * prod_{q > p} c_q (the last position runs fastest) and is alt[0][d_0] || ... || alt[P - 1][d_{P - 1}].  Packed, little-endian:
       u8 magic[4] = "GEN\0";  u8 npos;  u8 zero[3];  u32 nalt;  u32 pool_bytes;
       { u32 count; u32 first; } pos[npos]    first = index of the position's first alternative: positions in order, contiguous
       { u32 off;  u32 len;   } alt[nalt]     off into the pool
       u8 pool[pool_bytes]
   A malformed template (wrong magic, a zero byte that is not zero, counts that do not add up to nalt, an alternative outside the pool,
   a length that is not 16 + 8 npos + 8 nalt + pool_bytes, a limit above exceeded), T >= 2^64 and first + n > T are ECL_E_ARG with a
   message in ecl_hip_last_error, and nothing is launched.  The template goes to the device when it differs from the one the context
   holds (the context keeps a copy and compares); a call with the same template sends its first index alone.  Everything around the
   text - pieces, coverage, overflow, ecl_hip_fetch_found, the list confirm - is as on the context without the flag, and so is every
   other call.  ecl_hip_selftest of such a context also expands a built-in template against literal strings (ECL_E_SELFTEST). */
#define ECL_ADDR33 1u
#define ECL_ADDR65 2u
#define ECL_ENDO 4u
#define ECL_P2SH 16u
#define ECL_ETH 64u
#define ECL_TR 128u
#define ECL_PUB 256u
#define ECL_ORIGIN 512u
#define ECL_INSERT 1024u
#define ECL_HERD 2048u
#define ECL_PREFIX 4096u
#define ECL_MASK 0x2000u /* 8192 */
#define ECL_KDF_KECCAK 0x4000u /* 16384 */
#define ECL_KDF_SHA3 0x8000u   /* 32768 */
#define ECL_KDF_CAMP2 0xC000u  /* both: the two bits are one field */
#define ECL_KDF_BIP39 0x10000u /* 65536 */
#define ECL_GEN 0x20000u       /* 131072 */

/* return codes */
#define ECL_OK 0
#define ECL_E_ARG (-1)      /* bad argument */
#define ECL_E_HIP (-2)      /* HIP runtime error: ecl_hip_last_error() has the text */
#define ECL_E_NODEV (-3)    /* no such device / no gfx950 code object for it */
#define ECL_E_OVERFLOW (-4) /* more hits than `cap`: *nout = total hits, only `cap` records were written (the rest: ecl_hip_fetch_found) */
#define ECL_E_NOBLOOM (-5)  /* add/mul called before ecl_hip_set_bloom */
#define ECL_E_RANGE (-6)    /* range touches the scalar 0 (mod n) neighbourhood the method cannot represent */
#define ECL_E_SELFTEST (-7) /* the device code failed its known-answer / cross-path self-test (miscompile, bad GPU) */
#define ECL_E_COVERAGE (-8) /* the device did not hash every key of the call (section 1): no records, the call has to be repeated */

/* One bloom-filter hit.  key_offset counts keys from the `start` scalar of the call in units of the stride:
   privkey = start + key_offset * 2^ord_offs (mod n), then the endo map of calc_priv (main.c:267-276):
   endo 0: k, 1: -k, 2: k*lambda, 3: -k*lambda, 4: k*lambda^2, 5: -k*lambda^2.
   For ecl_hip_mul_batch key_offset is the index into the scalar array and endo is 0.
   h160 uses the reference's h160_t convention (addr.c:16): word i = digest bytes 4i..4i+3, big-endian. */
typedef struct ecl_found {
  uint64_t key_offset;
  uint32_t h160[5];
  uint8_t endo;
  uint8_t compressed; /* the address type: 1 = addr33, 0 = addr65, 2 = P2SH-P2WPKH (only for a context opened with ECL_P2SH),
                         3 = Ethereum (ECL_ETH; h160 holds the address), 4 = Taproot (ECL_TR, label p2tr; h160 holds the leading
                         20 bytes of the output key), 5 = public key (ECL_PUB, label pub; h160 holds the leading 20 bytes of x),
                         6 = distinguished point (ECL_HERD, label dp; the fields as the flags' comment gives them) */
  uint8_t pad[2];
} ecl_found; /* 32 bytes */

/* ==== 1. THE SEAM: what a binding of the reference's host program calls (INTEGRATION.md shows it: six one-line edits of main.c) ====
   device_count / open / set_bloom / add_range / mul_batch / close replace the reference's calls listed above; fetch_found serves a call
   whose hits did not fit the caller's buffer; strerror / last_error give the text of a failure.  Everything after this section is
   optional: a caller that uses nothing else gets the full search path, at the library's rate (the look-ahead of section 3 is on by
   default).
   Key coverage.  The kernels count, on the device, the keys (add) and scalars (mul) that reach the hash-and-probe step, and every
   add_range / mul_batch / mul_batch_raw call compares that count with what it asked for.  A call whose count differs returns
   ECL_E_COVERAGE (-8): *nout = 0, nothing is left for fetch_found, and the context re-positions its walk on the next call.  A call
   answered from a look-ahead sweep is covered by that sweep's count; a sweep that miscounts is never used, and the call that ran it
   returns ECL_E_COVERAGE.  The reference cannot tell that a key was never hashed (pk_verify_hash, main.c:248-263, only re-derives the
   hits that were reported), so a binding that treats every non-OK return as fatal - as the reference's own call sites do - stops here:
   that is the point.  On a sound device the code never occurs; ecl_hip_get_coverage (section 4) gives the totals. */
int ecl_hip_device_count(void);

/* Create a context on `device`. ord_offs: stride between consecutive keys is 2^ord_offs (0..255, main.c:221-222).
   On ECL_E_ARG / ECL_E_NODEV *out is untouched.  On any later failure (ECL_E_HIP, ECL_E_SELFTEST) *out holds a context
   that can only be asked for ecl_hip_last_error() and must be given to ecl_hip_close(). */
int ecl_hip_open(ecl_hip **out, int device, uint32_t flags, uint32_t ord_offs);
void ecl_hip_close(ecl_hip *h);

/* Copy the bloom bit array (little-endian u64 words, exactly the payload of a .blf file / of the in-memory
   filter built from a hash list, utils.c:277-280) into HBM.  May be called again to replace the filter. */
int ecl_hip_set_bloom(ecl_hip *h, const uint64_t *bits, uint64_t nwords);

/* Hash the nkeys keys  start, start+s, ..., start+(nkeys-1)*s  (s = 2^ord_offs; every encoding / endo variant
   selected at open) and report every bloom hit.  start: 256-bit scalar, 4 little-endian u64 limbs, as `fe` (a context opened with
   ECL_ORIGIN: twelve limbs - the scalar, then x and y of the origin point; with ECL_HERD: sixteen limbs and nkeys jumps; see the flags).
   Exactly these keys are tested - the caller reproduces the reference's job rounding (main.c:442,368).
   Consecutive calls whose `start` continues the previous range reuse the on-device walk state; small ones are answered from a
   look-ahead sweep (ecl_hip_set_lookahead) - same records either way.
   Returns ECL_OK, ECL_E_OVERFLOW (see above) or an error; ECL_E_ARG for an nkeys the geometry cannot walk in one call
   (more than 2^63, or more than 2^32 groups per lane - only reachable with a tiny caller-set geometry). */
int ecl_hip_add_range(ecl_hip *h, const uint64_t start[4], uint64_t nkeys, ecl_found *out, uint32_t cap,
                      uint32_t *nout);

/* `mul` command body (main.c:530-534): public keys of n scalars, hash, probe; key_offset = scalar index.
   The fixed-base window table of ec_gtable_mul (lib/ecc.c:876-929) is built on the device at a window width sized for
   HBM rather than for a CPU cache (the reference: 14 bits, 19.9 MB), with signed digits (a row holds 2^(W-1) points, a digit above
   2^(W-1) adds the negated point and carries): a context starts on 22 bits (12 rows, 11 * 2^21 + 2^14 points of 64 bytes = 1.5 GB,
   ~40 ms with the first call) and moves to 26 bits (10 rows, 19.6 GB, ~90 ms: 10 additions per scalar instead of 19) once it has
   multiplied 2^30 scalars, which is when the wider table has paid for its build (any width 8...29 can be fixed with
   ecl_hip_set_mul_window; 29 bits = 9 additions per scalar from a 138 GB table, for runs of 10^11 scalars and more).  A table is checked against the double-and-add kernel
   on sample slots before use (ECL_E_SELFTEST on a mismatch), shared between the contexts of a device in the process
   and freed with the last of them.  Results do not depend on the width. */
int ecl_hip_mul_batch(ecl_hip *h, const uint64_t (*scalars)[4], uint32_t n, ecl_found *out, uint32_t cap,
                      uint32_t *nout);
/* The records of the LAST ecl_hip_add_range / ecl_hip_mul_batch(_raw) call of this context that did not fit its `out`: a call
   keeps up to max(cap, 2^20) records on the device (32 MB), so after ECL_E_OVERFLOW (*nout = total > cap) the caller reads
   records [first, first + n) - the call itself delivered [0, cap) - instead of repeating a launch that may have walked
   2^32 keys.  *got = records written to `out` (fewer than n only if the call produced more than the device kept, i.e. more
   than max(cap, 2^20): then - and only then - the call has to be repeated with cap = total, as before).  Valid until the
   next add / mul call on the context.  The reference has no counterpart: its sink writes every hit as it is found
   (ctx_write_found, main.c:182-203), there is no buffer to overflow. */
int ecl_hip_fetch_found(ecl_hip *h, uint32_t first, ecl_found *out, uint32_t n, uint32_t *got);

const char *ecl_hip_strerror(int code);
const char *ecl_hip_last_error(const ecl_hip *h);

/* ==== 2. OPTIONAL: host-side steps of the path that can run on the device as well ====
   the exact list confirm (main.c:212-216), pk_verify_hash for a batch (main.c:248-263), `mul -raw`'s SHA-256 of the lines
   (main.c:505-527), load_filter's sort + bit setting for long lists (main.c:112-131), blf-gen's insert loop (utils.c:455-470);
   page-locked host memory for callers that feed `mul` */
/* Optional exact confirm on the device: the second half of ctx_check_hash (main.c:212-216).  h160 = the n sorted,
   unique list entries (ctx->to_find_hashes, order of compare_160, addr.c:18-26).  With a list resident, add_range /
   mul_batch report a hash only if it passed the bloom probe AND is in the list (a small kernel after the search
   kernel looks the bloom hits up by binary search; the list takes 20 bytes per entry of HBM); n = 0 removes the
   list again (bloom-only reporting).  ECL_E_ARG if the entries are not strictly increasing.  In list mode one call
   can stage max(cap, 2^20) bloom hits; beyond that it returns ECL_E_OVERFLOW with *nout = the number of bloom hits
   (and nothing to fetch: repeat the call with cap = *nout). */
int ecl_hip_set_list(ecl_hip *h, const uint32_t (*h160)[5], uint64_t n);

/* pk_verify_hash (main.c:248-263) for n reported private keys in one go: both hash160 values of k*G, derived on the
   device by a path other than the walk kernel (fixed-base window sum + own inversion per key).  The window sum and its
   table also give the base centre of a non-contiguous walk, and a hit shares its high digits with that centre, so
   the context self-test checks the window sum against the double-and-add kernel on full-width scalars.  ok[i] = 0
   for k = 0 (mod n).  The caller compares with the hit's h160 and treats a mismatch as fatal, like the reference.
   On a context opened with ECL_PREFIX | ECL_ORIGIN (or ECL_MASK | ECL_ORIGIN) each entry of `k` is TWELVE limbs, like the `start` of its ecl_hip_add_range: the
   scalar, then x and y of an origin O (a point of the curve, checked on the host: ECL_E_ARG otherwise; all eight limbs zero: the point at
   infinity), one origin per entry, and the hashes are those of O + k G - the window-table sum, one more complete mixed addition, an
   inversion of the kernel's own (k_verify_origin; ecl_hip_verify_eth: k_verify_origin_eth): not the walk.  ok[i] = 0 where O + k G is
   the point at infinity (k G = -O, or k = 0 (mod n) with O at infinity), in no other case.  n <= 2^24 there.  The image `endo` of a
   walked point O + k G is O' + k' G with k' = calc_priv(k, endo) and O' the same image of O, so a hit with endo != 0 is verified by
   the entry (k', O').  Every other context takes four limbs per entry, as always. */
int ecl_hip_verify(ecl_hip *h, const uint64_t (*k)[4], uint32_t n, uint32_t (*h33)[5], uint32_t (*h65)[5], uint8_t *ok);
/* ... and its P2SH half: out[i] = hash160(0x00 0x14 || h33[i]), the P2SH-P2WPKH hash of a key whose addr33 hash is h33[i] (both in
   h160_t words), computed on the device by the hash function of the search kernels.  A caller verifies a type-2 hit by passing the h33 of
   ecl_hip_verify through this.  Any context can be asked, whatever its flags. */
int ecl_hip_p2sh_hash(ecl_hip *h, const uint32_t (*h33)[5], uint32_t (*out)[5], uint32_t n);
/* ... and its ETH half: addr[i] = the Ethereum address (h160_t words) of k[i]*G by ecl_hip_verify's path (window-table sum + own inversion,
   not the walk kernel), ok[i] = 0 for k = 0 (mod n).  A caller verifies a type-3 hit with it.  Any context can be asked, whatever its flags. */
int ecl_hip_verify_eth(ecl_hip *h, const uint64_t (*k)[4], uint32_t n, uint32_t (*addr)[5], uint8_t *ok);

/* ... and its Taproot half: qx[i] = the 32-byte output key of k[i] as eight big-endian words (the h160_t convention continued: word j =
   bytes 4j..4j+3), by ecl_hip_verify's path (the 14-bit window table and an inversion of its own per key, for k G and again for
   t G + P' - not the search kernels); ok[i] = 0 for k = 0 (mod n) or t >= n.  A caller verifies a type-4 hit by comparing the first five
   words with the record's h160.  Any context can be asked, whatever its flags. */
int ecl_hip_verify_tr(ecl_hip *h, const uint64_t (*k)[4], uint32_t n, uint32_t (*qx)[8], uint8_t *ok);

/* `mul -raw` (main.c:505-527: the scalar of a line is the SHA-256 of its bytes, read as a big-endian number): the same as
   ecl_hip_mul_batch with the hashing done on the device.  `text` holds the lines' bytes (anywhere, in any order, newline
   bytes or not), lines[i] = offset of line i in `text` (low 32 bits) | its length in bytes (high 32 bits); n <= 2^26 lines
   and text_bytes < 2^32 - 16 per call, every line inside the text (ECL_E_ARG otherwise).  key_offset of a hit = line
   index; the caller re-derives that line's private key (one SHA-256) for the found record.  Page-locked `text` / `lines`
   arrays are read by DMA directly; a call is pipelined like ecl_hip_mul_batch's (the table and the hashing piece by piece), so large
   calls (2^24 lines) run at the rate of large ecl_hip_mul_batch calls.  On a context opened with ECL_KDF_KECCAK, ECL_KDF_SHA3 or
   ECL_KDF_CAMP2 the digest is that function's instead of SHA-256's (see the flags), and so is the key the caller re-derives. */
int ecl_hip_mul_batch_raw(ecl_hip *h, const uint8_t *text, uint32_t text_bytes, const uint64_t *lines, uint32_t n, ecl_found *out,
                          uint32_t cap, uint32_t *nout);

/* load_filter's list preparation (main.c:112-124: qsort by compare_160, then duplicates removed - the same here) on the device:
   sorts the n entries of h160 in place into compare_160 order (addr.c:18-26: word by word), removes duplicates, *kept =
   entries left at the front of the array.  (Five stable 32-bit radix sorts of an index permutation, least significant word first,
   then adjacent-duplicate flags, a scan and a scatter: this library's own kernels, off the hot path - a list is prepared once per
   run.)  n < 2^31.  10^7 entries: 13 s of qsort + bit setting on the host, 0.05 s here (the bits: ecl_hip_set_bloom of a zero filter + ecl_hip_bloom_insert + ecl_hip_get_bloom). */
int ecl_hip_sort_list(ecl_hip *h, uint32_t (*h160)[5], uint64_t n, uint64_t *kept);

/* blf_add (utils.c:290-306) in bulk: set the 20 bits of each of n hash160 values (h160_t words) in the resident
   filter; ecl_hip_get_bloom copies the bit array back (e.g. to write a .blf file, utils.c:328-360). */
int ecl_hip_bloom_insert(ecl_hip *h, const uint32_t (*h160)[5], uint64_t n);
int ecl_hip_get_bloom(ecl_hip *h, uint64_t *bits, uint64_t nwords);
/* The insert loop of blf-gen (utils.c:455-470) for n hashes in input order: a hash that blf_has already reports at its
   turn is skipped; *added = the number that were new - the reference's "added N new items", exact also for duplicate
   and colliding hashes (the bits are those of ecl_hip_bloom_insert). */
int ecl_hip_bloom_insert_count(ecl_hip *h, const uint32_t (*h160)[5], uint64_t n, uint64_t *added);

/* Page-locked host memory (hipHostMalloc / hipHostFree): scalar arrays given to ecl_hip_mul_batch from such memory are read by the
   GPU's copy engine directly (57 GB/s), pageable ones go through a staging copy (18 GB/s: 0.57 instead of 1.3 G scalars/s for `mul`).
   The runtime places the pages next to the GPU, which matters on a two-socket host: from the far socket the copy runs at about half
   the rate (30 against 57 GB/s measured).  (There is no call that page-locks the caller's own memory in place: register / unregister
   cycles on memory the host allocator recycles fault inside the ROCm runtime - profiles/r05_pin_fault.txt.) */
void *ecl_hip_alloc_host(size_t bytes);
void ecl_hip_free_host(void *p);

/* ==== 3. TUNING: none of these changes a result ==== */
/* Optional: allocate now what a later ecl_hip_add_range of `nkeys` keys with record capacity `cap` will need (table,
   lane centres, prefix-product chains, record buffer), so that the first call does not pay for it.  The reference has
   no counterpart (its per-thread buffers live on the stack, main.c:350-352).  On a Taproot context also the slab and the `mul` table. */
int ecl_hip_reserve(ecl_hip *h, uint64_t nkeys, uint32_t cap);

/* Optional: set up now what a later ecl_hip_mul_batch of up to n scalars with record capacity `cap` needs (the window
   table of the width in force, device staging, record buffer), so that the first batch does not pay for it - the
   counterpart of ecl_hip_reserve for `mul`; the reference builds its table at the start of cmd_mul (main.c:543). */
int ecl_hip_reserve_mul(ecl_hip *h, uint32_t n, uint32_t cap);

/* Look-ahead over small contiguous jobs.  The reference's scheduler hands out jobs of 2^21 keys (MAX_JOB_SIZE, main.c:16,418-431): 0.17 ms
   of work for this GPU, where a launch needs 2^28 keys and more to reach the kernel's rate.  When the ecl_hip_add_range calls of the
   contexts that share a filter (same flags - so a context with ECL_P2SH or ECL_ETH never shares a sweep with one without it -, stride and filter
   contents, any device) form that pattern - equal sizes, each starting where
   the one before ended - a call that finds nothing prepared runs ONE sweep of up to `max_keys` keys from its start, keeps the sweep's hit
   records on the host and the following calls are answered from them without a launch: each call still receives exactly the hits of its
   own keys, with key_offset counted from its own start.  Default 2^30 keys (environment ECL_HIP_LOOKAHEAD_LOG2=N, 0 = off);
   max_keys = 0 turns it off for this context, else 2^22 <= max_keys <= 2^32.  Calls larger than max_keys / 4, contexts with a
   caller-set geometry (ecl_hip_set_geometry) and filters changed on the device (ecl_hip_bloom_insert) are never looked ahead for. */
int ecl_hip_set_lookahead(ecl_hip *h, uint64_t max_keys);
/* Optional hint: the scalar at which the caller's scan stops handing out jobs (ctx->range_e: a worker stops once range_s >= range_e,
   main.c:420-423); NULL withdraws it.  A sweep then never passes the job that contains `end` - nothing is computed that will not be asked
   for - and starts with the second contiguous job; without the hint a sweep covers at most half of what the pattern has consumed so far.
   Either way a sweep is only run if it replaces at least 4 jobs per context of the group (N equal shards handed to N GPUs stay N launches). */
int ecl_hip_set_scan_end(ecl_hip *h, const uint64_t end[4]);
/* Measurement: sweeps this context has run and their keys; calls answered from a sweep (this context's or a sharing one's) and their keys. */
int ecl_hip_get_lookahead_stats(ecl_hip *h, uint64_t *sweeps, uint64_t *swept_keys, uint64_t *served_calls, uint64_t *served_keys);

/* Optional: fix the window width of this context's `mul` table (8..29 bits; 0 = automatic, the default) from the next
   ecl_hip_mul_batch on - a caller that knows it will multiply billions of scalars takes 22 at once.  No reference
   counterpart other than the compile-time _GTABLE_W (lib/ecc.c:876). */
int ecl_hip_set_mul_window(ecl_hip *h, uint32_t bits);
/* ... and the width of the table the context holds right now (0: none yet). */
int ecl_hip_get_mul_window(ecl_hip *h, uint32_t *bits);

/* Geometry of the walk: half_group = table points per group (the reference fixes 1024: GROUP_INV_SIZE/2,
   main.c:17), max_lanes = keys walked concurrently.  0 keeps the default (1024 and 2^21 lanes; the walk parks
   lanes * half_group * 36 bytes of prefix products in HBM - 77 GB at the default - and takes fewer lanes by itself
   when free memory is short; while half_group is left at its default, calls shorter than lanes * 2048 keys use a half
   group of 512 or 256 so that the lanes stay oversubscribed).  Results do not depend on either. */
int ecl_hip_set_geometry(ecl_hip *h, uint32_t half_group, uint32_t max_lanes);
/* Current geometry.  One "sweep" = lanes * 2 * half_group keys: calls whose nkeys is a multiple of it keep every
   lane equally busy (no tail) and can be continued by the next contiguous call without re-initialisation. */
int ecl_hip_get_geometry(ecl_hip *h, uint32_t *half_group, uint32_t *lanes);

/* The geometry ecl_hip_add_range would walk a call of `nkeys` keys with: half group, lanes, groups per lane.  While the half group is
   left automatic it follows a measured cost model (one inversion per lane and group against keeping the chip oversubscribed):
   8 x 2^17 lanes for the reference's 2^21-key job, 32 x 2^18 for 2^24 keys, 128 x 2^21 for 2^29, 1024 x 2^21 for 2^32.  Contiguous
   calls continue the resident walk only while this stays the same, i.e. for calls of one size. */
int ecl_hip_plan_geometry(ecl_hip *h, uint64_t nkeys, uint32_t *half_group, uint32_t *lanes, uint32_t *groups_per_lane);

/* ==== 4. MEASUREMENT ==== */
/* Measurement: accumulated HIP-event time of the main add kernel since the last reset, and launch count (Taproot: of both stages of
   every slab, one launch counted per slab). */
int ecl_hip_get_timing(ecl_hip *h, double *kernel_ms, uint64_t *launches, uint64_t *keys);
int ecl_hip_reset_timing(ecl_hip *h);
/* ... of the set-up a non-contiguous ecl_hip_add_range pays before its search kernel (base centre through the window
   table, lane centres; HIP events on the handle's stream), and how many calls paid it; contiguous follow-up calls
   pay nothing.  Reset by ecl_hip_reset_timing. */
int ecl_hip_get_setup_timing(ecl_hip *h, double *setup_ms, uint64_t *setups);
/* ... of ecl_hip_mul_batch: HIP-event time from the first chunk's copy being awaited to the last kernel (host->device
   copies overlapped with the kernels), calls and scalars since the last reset. */
int ecl_hip_get_mul_timing(ecl_hip *h, double *ms, uint64_t *calls, uint64_t *scalars);
/* Coverage totals since open: requested = keys (add) and scalars (mul) of the calls that launched or were served from a sweep;
   covered = those whose device count was checked equal to what was asked (by their own launch or by the sweep that held them);
   device = keys counted by the kernels of this context's own launches, sweeps whole (so >= covered with the look-ahead on).
   On a sound device requested == covered always.  Not reset by ecl_hip_reset_timing; the self-test's launches are left out. */
int ecl_hip_get_coverage(ecl_hip *h, uint64_t *requested, uint64_t *covered, uint64_t *device_keys);

/* Known-answer test of the device code (hash160 of 1*G, 2*G, 0xdc2a04*G, both encodings, via the double-and-add
   kernel; the P2SH-P2WPKH hash and the Ethereum address of 1*G) and a cross-check of the walk kernel against it over 4096 consecutive
   keys (with ECL_P2SH: the script hashes too; with ECL_ETH: the Ethereum addresses, against ecl_hip_verify_eth; with ECL_TR: the output
   keys, against ecl_hip_verify_tr; with ECL_PUB: the leading 20 bytes of x of the double-and-add kernel's points), and the Taproot output keys of the three private keys (ecl_hip_verify_tr).  ecl_hip_open() runs it
   (a few ms) unless the environment has ECL_HIP_SKIP_SELFTEST=1; a failure makes open return ECL_E_SELFTEST. */
int ecl_hip_selftest(ecl_hip *h);

/* ==== 5. DIAGNOSTICS: device primitives exposed for the parity tests (each runs a tiny kernel); not for production callers ==== */
/* op: 0 mul, 1 sqr, 2 inv (the one the kernels use), 3 sub, 4 add, 5 neg, 6 sqr(sqr a), 7 (a*b)*b, 8 sqr(a)*a, 9 inv by division steps,
   10 inv by the addition chain of lib/ecc.c:463-520, 11 1 / (4b - 2a) by division steps from an unnormalised operand; a,b,r: n field
   elements as 4 little-endian u64 limbs */
int ecl_hip_diag_fe(ecl_hip *h, int op, const uint64_t (*a)[4], const uint64_t (*b)[4], uint64_t (*r)[4], uint32_t n);
/* one field or point function on RAW LIMBS (9 limbs of 29 bits per element, nothing normalised on the way in or out), for the tests at
   the limits of the magnitude contract: op = an operation of csrc/limb_ops.h (the list is written there only), in = n cases of up to six
   input elements, out = up to four result elements per case (unused ones zero), flag = a result word per case (parity, is-zero,
   infinity).  The caller keeps every limb inside the magnitude the function documents; an unknown op is ECL_E_ARG. */
int ecl_hip_diag_limbs(ecl_hip *h, int op, const uint32_t (*in)[6][9], uint32_t (*out)[4][9], uint32_t *flag, uint32_t n);
/* affine public keys of n scalars (double-and-add kernel); ok[i] = 0 for the point at infinity */
int ecl_hip_diag_mulg(ecl_hip *h, const uint64_t (*k)[4], uint64_t (*x)[4], uint64_t (*y)[4], uint8_t *ok, uint32_t n);
/* hash160 of n affine points, both encodings */
int ecl_hip_diag_hash160(ecl_hip *h, const uint64_t (*x)[4], const uint64_t (*y)[4], uint32_t (*h33)[5],
                         uint32_t (*h65)[5], uint32_t n);
/* bloom probe of n hashes against the resident filter */
int ecl_hip_diag_bloom(ecl_hip *h, const uint32_t (*h160)[5], uint8_t *hit, uint32_t n);
/* the probe's word index r[i] = x[i] mod nwords (the `% (blf->size * 64)` of utils.c:286-288 on the word index) as the
   device computes it, for any filter size 0 < nwords < 2^58 and x < 2^58; no filter needs to be resident */
int ecl_hip_diag_bloom_mod(ecl_hip *h, uint64_t nwords, const uint64_t *x, uint64_t *r, uint32_t n);
/* one-shot: the next search launch of this context (add_range, a look-ahead sweep, or the first piece of a mul call) runs one
   round short - add: groups per lane nb - 1, mul: scalars per thread R - 1 - so that keys of the call are silently not hashed
   (the call then returns ECL_E_COVERAGE: the check of section 1, under test).  Only a loop bound shrinks. */
int ecl_hip_diag_drop_round(ecl_hip *h);
/* Taproot: the search path's two stages for n AFFINE POINTS (x, y on the curve) instead of keys - stage A's even-y lift and tweak, stage B's
   window sum, addition and normalisation (k_tr_check) - so that a published vector whose private key nobody has runs on the device code
   of the search: t[i] = the tweak of x[i], qx[i] = the output key (eight big-endian words), ok[i] = 0 where there is none.  n <= 2^20. */
int ecl_hip_diag_tr(ecl_hip *h, const uint64_t (*x)[4], const uint64_t (*y)[4], uint64_t (*t)[4], uint32_t (*qx)[8], uint8_t *ok, uint32_t n);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
