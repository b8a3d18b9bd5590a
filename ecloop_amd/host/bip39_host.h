/* bip39_host.h - the host program's own BIP39 / BIP32 derivation: SHA-512 (FIPS 180-4), HMAC (RFC 2104), PBKDF2 (RFC 8018) and CKDpriv
   (BIP32) in plain C on bytes and 64-bit words, written apart from the device code (csrc/sha512.h, csrc/bip39.h) as keccak_host.h is from
   kdf.h: `seed` recomputes every hit's key with it, so a key is printed only where two implementations agree.  The public key of a normal
   (not hardened) path element is not computed here: the caller supplies it (cli_seed.h asks the device's double-and-add kernel).
   Part of the one translation unit ecloop_hip_cli.c. */
#define B32_HARDENED 0x80000000u
#define B32_DEPTH_MAX 10
#define B39_PASS_MAX 99

static const u64 B39_K[80] = {
    0x428a2f98d728ae22ULL, 0x7137449123ef65cdULL, 0xb5c0fbcfec4d3b2fULL, 0xe9b5dba58189dbbcULL, 0x3956c25bf348b538ULL, 0x59f111f1b605d019ULL,
    0x923f82a4af194f9bULL, 0xab1c5ed5da6d8118ULL, 0xd807aa98a3030242ULL, 0x12835b0145706fbeULL, 0x243185be4ee4b28cULL, 0x550c7dc3d5ffb4e2ULL,
    0x72be5d74f27b896fULL, 0x80deb1fe3b1696b1ULL, 0x9bdc06a725c71235ULL, 0xc19bf174cf692694ULL, 0xe49b69c19ef14ad2ULL, 0xefbe4786384f25e3ULL,
    0x0fc19dc68b8cd5b5ULL, 0x240ca1cc77ac9c65ULL, 0x2de92c6f592b0275ULL, 0x4a7484aa6ea6e483ULL, 0x5cb0a9dcbd41fbd4ULL, 0x76f988da831153b5ULL,
    0x983e5152ee66dfabULL, 0xa831c66d2db43210ULL, 0xb00327c898fb213fULL, 0xbf597fc7beef0ee4ULL, 0xc6e00bf33da88fc2ULL, 0xd5a79147930aa725ULL,
    0x06ca6351e003826fULL, 0x142929670a0e6e70ULL, 0x27b70a8546d22ffcULL, 0x2e1b21385c26c926ULL, 0x4d2c6dfc5ac42aedULL, 0x53380d139d95b3dfULL,
    0x650a73548baf63deULL, 0x766a0abb3c77b2a8ULL, 0x81c2c92e47edaee6ULL, 0x92722c851482353bULL, 0xa2bfe8a14cf10364ULL, 0xa81a664bbc423001ULL,
    0xc24b8b70d0f89791ULL, 0xc76c51a30654be30ULL, 0xd192e819d6ef5218ULL, 0xd69906245565a910ULL, 0xf40e35855771202aULL, 0x106aa07032bbd1b8ULL,
    0x19a4c116b8d2d0c8ULL, 0x1e376c085141ab53ULL, 0x2748774cdf8eeb99ULL, 0x34b0bcb5e19b48a8ULL, 0x391c0cb3c5c95a63ULL, 0x4ed8aa4ae3418acbULL,
    0x5b9cca4f7763e373ULL, 0x682e6ff3d6b2b8a3ULL, 0x748f82ee5defb2fcULL, 0x78a5636f43172f60ULL, 0x84c87814a1f0ab72ULL, 0x8cc702081a6439ecULL,
    0x90befffa23631e28ULL, 0xa4506cebde82bde9ULL, 0xbef9a3f7b2c67915ULL, 0xc67178f2e372532bULL, 0xca273eceea26619cULL, 0xd186b8c721c0c207ULL,
    0xeada7dd6cde0eb1eULL, 0xf57d4f7fee6ed178ULL, 0x06f067aa72176fbaULL, 0x0a637dc5a2c898a6ULL, 0x113f9804bef90daeULL, 0x1b710b35131c471bULL,
    0x28db77f523047d84ULL, 0x32caab7b40c72493ULL, 0x3c9ebe0a15c9bebcULL, 0x431d67c49c100d4cULL, 0x4cc5d4becb3e42b6ULL, 0x597f299cfc657e2aULL,
    0x5fcb6fab3ad6faecULL, 0x6c44198c4a475817ULL};

typedef struct { u64 h[8]; u8 buf[128]; size_t fill; u64 total; } b39_sha512;
static inline u64 b39_ror(u64 x, int n) { return x >> n | x << (64 - n); }
static void b39_block(u64 h[8], const u8 *p) {
  u64 w[80], s[8];
  for (int i = 0; i < 16; ++i) {
    w[i] = 0;
    for (int j = 0; j < 8; ++j) w[i] = w[i] << 8 | p[8 * i + j];
  }
  for (int i = 16; i < 80; ++i)
    w[i] = w[i - 16] + (b39_ror(w[i - 15], 1) ^ b39_ror(w[i - 15], 8) ^ w[i - 15] >> 7) + w[i - 7] + (b39_ror(w[i - 2], 19) ^ b39_ror(w[i - 2], 61) ^ w[i - 2] >> 6);
  memcpy(s, h, sizeof s);
  for (int i = 0; i < 80; ++i) {
    const u64 t1 = s[7] + (b39_ror(s[4], 14) ^ b39_ror(s[4], 18) ^ b39_ror(s[4], 41)) + ((s[4] & s[5]) ^ (~s[4] & s[6])) + B39_K[i] + w[i];
    const u64 t2 = (b39_ror(s[0], 28) ^ b39_ror(s[0], 34) ^ b39_ror(s[0], 39)) + ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
    memmove(s + 1, s, 7 * sizeof s[0]);
    s[4] += t1, s[0] = t1 + t2;
  }
  for (int i = 0; i < 8; ++i) h[i] += s[i];
}
static void b39_init(b39_sha512 *c) {
  static const u64 IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                            0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
  memcpy(c->h, IV, sizeof IV), c->fill = 0, c->total = 0;
}
static void b39_update(b39_sha512 *c, const u8 *p, size_t n) {
  c->total += n;
  while (n) {
    const size_t take = 128 - c->fill < n ? 128 - c->fill : n;
    memcpy(c->buf + c->fill, p, take), c->fill += take, p += take, n -= take;
    if (c->fill == 128) b39_block(c->h, c->buf), c->fill = 0;
  }
}
static void b39_final(b39_sha512 *c, u8 out[64]) {
  const u64 bits = c->total * 8;
  u8 pad[256] = {0x80};
  const size_t padlen = (c->fill < 112 ? 112 : 240) - c->fill;
  for (int i = 0; i < 8; ++i) pad[padlen + 8 + i] = (u8)(bits >> (56 - 8 * i)); /* (the high length word stays zero) */
  b39_update(c, pad, padlen + 16);
  for (int i = 0; i < 64; ++i) out[i] = (u8)(c->h[i / 8] >> (56 - 8 * (i % 8)));
}
typedef struct { b39_sha512 in, out; } b39_hmac;
static void b39_hmac_key(b39_hmac *m, const u8 *key, size_t klen) {
  u8 k[128] = {0}, pad[128];
  if (klen > 128) {
    b39_sha512 c;
    b39_init(&c), b39_update(&c, key, klen), b39_final(&c, k);
  } else memcpy(k, key, klen);
  for (int i = 0; i < 128; ++i) pad[i] = k[i] ^ 0x36;
  b39_init(&m->in), b39_update(&m->in, pad, 128);
  for (int i = 0; i < 128; ++i) pad[i] = k[i] ^ 0x5c;
  b39_init(&m->out), b39_update(&m->out, pad, 128);
}
static void b39_hmac_of(const b39_hmac *m, const u8 *msg, size_t n, u8 out[64]) {
  b39_sha512 c = m->in;
  u8 inner[64];
  b39_update(&c, msg, n), b39_final(&c, inner);
  c = m->out;
  b39_update(&c, inner, 64), b39_final(&c, out);
}
/* BIP39: PBKDF2-HMAC-SHA512(phrase, "mnemonic" || pass, 2048, 64 bytes) - one block */
static void b39_seed(u8 seed[64], const u8 *phrase, size_t plen, const u8 *pass, size_t pass_len) {
  b39_hmac m;
  u8 salt[8 + B39_PASS_MAX + 4], u[64];
  b39_hmac_key(&m, phrase, plen);
  memcpy(salt, "mnemonic", 8), memcpy(salt + 8, pass, pass_len);
  salt[8 + pass_len] = salt[9 + pass_len] = salt[10 + pass_len] = 0, salt[11 + pass_len] = 1;
  b39_hmac_of(&m, salt, 12 + pass_len, u);
  memcpy(seed, u, 64);
  for (int it = 1; it < 2048; ++it) {
    b39_hmac_of(&m, u, 64, u);
    for (int i = 0; i < 64; ++i) seed[i] ^= u[i];
  }
}
static sc b32_sc_of(const u8 b[32]) {
  sc k;
  for (int i = 0; i < 4; ++i) {
    k.w[3 - i] = 0;
    for (int j = 0; j < 8; ++j) k.w[3 - i] = k.w[3 - i] << 8 | b[8 * i + j];
  }
  return k;
}
static void b32_bytes_of(u8 b[32], const sc *k) {
  for (int i = 0; i < 32; ++i) b[i] = (u8)(k->w[3 - i / 8] >> (56 - 8 * (i % 8)));
}
/* the master node of a seed -> false for an invalid one */
static bool b32_master(sc *k, u8 c[32], const u8 seed[64]) {
  b39_hmac m;
  u8 I[64];
  b39_hmac_key(&m, (const u8 *)"Bitcoin seed", 12);
  b39_hmac_of(&m, seed, 64, I);
  *k = b32_sc_of(I), memcpy(c, I + 32, 32);
  return !sc_is_zero(k) && sc_cmp(k, &SC_N) < 0;
}
/* CKDpriv.  pub33: the 33 bytes of serP(k G), read for a normal index only -> false for an invalid child */
static bool b32_ckd(sc *k, u8 c[32], u32 index, const u8 *pub33) {
  b39_hmac m;
  u8 data[37], I[64];
  if (index & B32_HARDENED) data[0] = 0, b32_bytes_of(data + 1, k);
  else memcpy(data, pub33, 33);
  data[33] = (u8)(index >> 24), data[34] = (u8)(index >> 16), data[35] = (u8)(index >> 8), data[36] = (u8)index;
  b39_hmac_key(&m, c, 32);
  b39_hmac_of(&m, data, 37, I);
  const sc il = b32_sc_of(I);
  if (sc_cmp(&il, &SC_N) >= 0) return false;
  const sc sum = sc_add(il, *k);
  if (sc_is_zero(&sum)) return false;
  *k = sum, memcpy(c, I + 32, 32);
  return true;
}
/* m/44'/0'/0'/0/0 (' or h: hardened) -> elements; -1 for a path that is not one, or deeper than 10 */
static int b32_parse_path(const char *s, u32 el[B32_DEPTH_MAX]) {
  if (s[0] != 'm') return -1;
  int depth = 0;
  for (const char *p = s + 1; *p;) {
    if (*p != '/' || depth == B32_DEPTH_MAX) return -1;
    ++p;
    if (*p < '0' || *p > '9') return -1;
    u64 v = 0;
    for (; *p >= '0' && *p <= '9'; ++p)
      if ((v = v * 10 + (u64)(*p - '0')) >= B32_HARDENED) return -1;
    u32 e = (u32)v;
    if (*p == '\'' || *p == 'h') e |= B32_HARDENED, ++p;
    el[depth++] = e;
  }
  return depth;
}
static void b32_format_path(char *dst, size_t cap, const u32 *el, int depth) {
  size_t at = (size_t)snprintf(dst, cap, "m");
  for (int i = 0; i < depth && at < cap; ++i) at += (size_t)snprintf(dst + at, cap - at, "/%u%s", el[i] & ~B32_HARDENED, el[i] & B32_HARDENED ? "'" : "");
}
