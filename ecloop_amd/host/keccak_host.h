/* keccak_host.h - the key derivation functions of `mul -raw -kdf` on the host: Keccak-256, SHA3-256 and the 2031-fold Keccak-256 of the
   ethercamp wallet (`camp2`), for re-deriving the key of a hit and for the hidden `parse` verb.  Plain C on 64-bit lanes, written from
   FIPS 202 (algorithms 1-7: theta, rho, pi, chi, iota step by step over a 5 x 5 array; algorithm 8: the sponge) and sharing nothing
   with the device code (csrc/keccak.h, csrc/kdf.h: 32-bit half lanes, fused steps): a device hash that disagrees with this one fails
   the re-verification of every hit instead of printing a wrong key.
   Part of the one translation unit ecloop_hip_cli.c (included there, in front of cli_mul.h). */
enum { KDF_SHA256 = 0, KDF_KECCAK = 1, KDF_SHA3 = 2, KDF_CAMP2 = 3 };
static const char *const KDF_NAMES[4] = {"sha256", "keccak", "sha3", "camp2"};
#define KDF_CAMP2_HASHES 2031

/* rc(t) of algorithm 5: the output bit of the LFSR x^8 + x^6 + x^5 + x^4 + 1 after t steps */
static int khost_rc_bit(int t) {
  unsigned r = 1;
  for (int i = 0; i < t % 255; ++i) {
    r <<= 1;
    if (r & 0x100) r ^= 0x171;
  }
  return r & 1;
}
static u64 khost_rotl(u64 v, int n) { return n ? (v << n) | (v >> (64 - n)) : v; }
/* round constants (algorithm 5) and rotation offsets (algorithm 2: (t + 1)(t + 2) / 2 along the orbit of (x, y) -> (y, 2x + 3y)); set once in main */
static u64 KHOST_RC[24];
static int KHOST_ROT[5][5];
static void khost_init(void) {
  for (int i = 0; i < 24; ++i) {
    u64 v = 0;
    for (int j = 0; j <= 6; ++j)
      if (khost_rc_bit(j + 7 * i)) v |= 1ull << ((1 << j) - 1);
    KHOST_RC[i] = v;
  }
  int x = 1, y = 0;
  KHOST_ROT[0][0] = 0;
  for (int t = 0; t < 24; ++t) {
    KHOST_ROT[x][y] = ((t + 1) * (t + 2) / 2) % 64;
    const int nx = y, ny = (2 * x + 3 * y) % 5;
    x = nx, y = ny;
  }
}
/* Keccak-f[1600] on a[x][y] */
static void khost_permute(u64 a[5][5]) {
  for (int rnd = 0; rnd < 24; ++rnd) {
    u64 c[5], d[5], b[5][5];
    for (int x = 0; x < 5; ++x) c[x] = a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4];
    for (int x = 0; x < 5; ++x) d[x] = c[(x + 4) % 5] ^ khost_rotl(c[(x + 1) % 5], 1);
    for (int x = 0; x < 5; ++x)
      for (int y = 0; y < 5; ++y) a[x][y] ^= d[x]; /* theta */
    for (int x = 0; x < 5; ++x)
      for (int y = 0; y < 5; ++y) b[y][(2 * x + 3 * y) % 5] = khost_rotl(a[x][y], KHOST_ROT[x][y]); /* rho, pi */
    for (int x = 0; x < 5; ++x)
      for (int y = 0; y < 5; ++y) a[x][y] = b[x][y] ^ (~b[(x + 1) % 5][y] & b[(x + 2) % 5][y]); /* chi */
    a[0][0] ^= KHOST_RC[rnd]; /* iota */
  }
}
/* the sponge with rate 136 and a 32-byte output: pad = 0x01 (Keccak-256) or 0x06 (SHA3-256) */
static void khost_sponge256(u8 out[32], const u8 *msg, size_t len, u8 pad) {
  u64 a[5][5];
  memset(a, 0, sizeof a);
  u8 blk[136];
  for (bool last = false; !last;) {
    if (len >= 136) {
      memcpy(blk, msg, 136), msg += 136, len -= 136;
    } else {
      memset(blk, 0, 136);
      if (len) memcpy(blk, msg, len);
      blk[len] ^= pad, blk[135] ^= 0x80;
      last = true;
    }
    for (int i = 0; i < 17; ++i) {
      u64 v = 0;
      for (int k = 7; k >= 0; --k) v = v << 8 | blk[8 * i + k];
      a[i % 5][i / 5] ^= v;
    }
    khost_permute(a);
  }
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 8; ++k) out[8 * i + k] = (u8)(a[i][0] >> (8 * k));
}
/* the digest of a line under -kdf keccak | sha3 | camp2 (sha256 is sha256_stream of cli_mul.h) */
static void kdf_host_digest(int kdf, u8 out[32], const u8 *msg, size_t len) {
  khost_sponge256(out, msg, len, kdf == KDF_SHA3 ? 0x06 : 0x01);
  if (kdf == KDF_CAMP2)
    for (int i = 1; i < KDF_CAMP2_HASHES; ++i) {
      u8 d[32];
      memcpy(d, out, 32);
      khost_sponge256(out, d, 32, 0x01);
    }
}
/* -kdf <name>: -> KDF_*, or -1 */
static int kdf_from_name(const char *name) {
  for (int i = 0; i < 4; ++i)
    if (!strcmp(name, KDF_NAMES[i])) return i;
  return -1;
}
