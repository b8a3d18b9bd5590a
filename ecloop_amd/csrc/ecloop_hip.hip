// ecloop_hip.hip — kernels' instantiation + the C ABI of include/ecloop_hip.h (host side, HIP runtime).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared ecloop_hip.hip -o libecloop_hip.so
#include "../../include/ecloop_hip.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "add_kernel.h"
#include "ec.h"
#include "scalar_host.h"
#include "abi_lookahead_ctx.h"
#include "setup_kernels.h"
#include "mul_kernels.h"
#include "kdf.h"
#include "tr_kernels.h"
#include "aux_kernels.h"
#include "herd_kernel.h"
#include "bip39.h"
#include "gen.h"
#include "../host/gen_plan.h"
#include "devbuf.h"
#include "callstate.h"

// the two kinds of memory the library owns (devbuf.h): device memory, and page-locked host memory for its own staging
struct dev_mem {
  typedef hipError_t error;
  static constexpr hipError_t ok = hipSuccess;
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
};
struct pin_mem {
  typedef hipError_t error;
  static constexpr hipError_t ok = hipSuccess;
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void* p) { (void)hipHostFree(p); }
};
template <typename T> using devbuf = growbuf<T, dev_mem>;
template <typename T> using pinbuf = growbuf<T, pin_mem>;

// ------------------------------------------------------------------------------------------------ context

#define ECL_AUX_WORDS (34u * 16u)  /* d_aux: 34 points; one word more behind them: k_origin_add's infinity flag (its host copy: pin_counter[CW_ORIGIN_INF]) */

struct ecl_hip {
  int dev = 0;
  u32 flags = 0, offs = 0;
  u32 kdf = 0;        // ECL_KDF_* of ecl_hip_open (not part of `flags`): the hash of ecl_hip_mul_batch_raw, 0 = SHA-256
  bool bip39 = false; // ECL_KDF_BIP39 of ecl_hip_open (not part of `flags` either): ecl_hip_mul_batch_raw derives BIP32 keys from phrases (abi_seed.h)
  u32 B = 1024;       // table points per group
  u32 Tmax = 0;       // lanes walked concurrently (0 = derive from occupancy)
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::string err;
  // device buffers (devbuf / pinbuf: each owns its memory and knows how many elements it holds; the context's destructor frees them)
  devbuf<u32> d_tab; u32 tab_B = 0;            // table for (B, offs): tab_B = the half group its contents were built for
  devbuf<u32> d_gtab;                          // fixed-base window table for `mul` (19 x 16383 affine points)
  devbuf<u32> d_aux;                           // [0]=C0, [1]=jump, [2..33]=ladder : 34 points x 16 words
  devbuf<u32> d_auxk;                          // scalars for the above
  devbuf<uint4> d_cxy;                         // lane centres: 4 per lane
  devbuf<uint4> d_ctab;                        // (g + 1) * D, g < T, for the geometry of d_aux (k_init_centres_table): 4 per lane
  bool ctab_valid = false;
  devbuf<uint4> d_scr; devbuf<u32> d_scr2;     // prefix-product chains (ensure_scratch)
  devbuf<u64> d_bloom; u64 bloom_words = 0;
  u32 mask_n = 0;    // ECL_MASK: d_bloom holds the table of mask_n entries (five 64-bit words each) and nothing else
  u32 prefix_n = 0;  // ECL_PREFIX: d_bloom holds the stage-1 bitmap (PREFIX_BITMAP_WORDS64 words) and behind it the table of prefix_n ranges
  // `mul`: scalars travel in pieces through MUL_NBUF device buffers (and as many pinned staging buffers for pageable callers), the copy
  // engine running up to MUL_NBUF - 1 pieces ahead of the kernel
  devbuf<u32> d_kbuf[MUL_NBUF]; pinbuf<u32> pin_k[MUL_NBUF]; u32 kbuf_cap = 0;  // kbuf_cap: scalars of a piece, once d_kbuf and d_multmp all hold them
  devbuf<u32> d_multmp[2];                     // parked window sums of one piece (144 bytes per scalar), one space per compute stream
  const u32* d_multab = nullptr; u32 multab_W = 0;  // `mul`'s window table in use: one per (device, width), shared by the contexts
  u32 mul_W_fixed = 0;                         // ecl_hip_set_mul_window: 0 = automatic
  uint64_t mul_seen = 0;                       // scalars this context has multiplied (never reset: the automatic width goes by it)
  bool mul_long_failed = false;                // the long table could not be allocated: do not try again
  devbuf<u8> d_ver;                            // staging of ecl_hip_verify: 76 bytes per scalar
  // Taproot (ECL_TR): the slab of `add` (t, P' of up to one slab of keys, 96 bytes each) and the parking space of its k_tr_check; one slab
  // per compute stream for the pieces of `mul`; the mark the next emit launch gives its entries (tr_emit)
  devbuf<u32> d_trslab, d_trtmp[2], d_trslab_mul[2];
  u32 tr_epoch = 0, tr_epoch_mul[2] = {};
  devbuf<u32> d_rawtext; devbuf<u64> d_rawlines;  // `mul -raw`: text and line table of one call
  // ECL_KDF_BIP39: the master nodes of the last reuse = 0 call (64 bytes per phrase), how many, their passphrase, and whether the call
  // before this one returned ECL_OK or ECL_E_OVERFLOW - what a reuse = 1 call is checked against
  devbuf<u32> d_nodes; u32 seed_n = 0, seed_pass_len = 0; uint8_t seed_pass[BIP39_PASS_MAX] = {};
  bool seed_have = false, seed_last_ok = false;
  // ECL_GEN (not part of `flags` either): ecl_hip_mul_batch_raw takes a template and generates the lines (abi_gen.h).  The template the device
  // holds in d_gen, as the caller gave it (gen_blob: what the next call's is compared with) and as it was sent (gen_img: lives until the copy is done)
  bool gen = false;
  devbuf<u32> d_gen; std::vector<uint8_t> gen_blob; std::vector<u32> gen_img;
  hipStream_t copy_stream = nullptr, stream2 = nullptr;  // `mul`: the copy engine's stream; the second compute stream (pieces alternate)
  hipEvent_t ev_copied[MUL_NBUF] = {}, ev_free[MUL_NBUF] = {}, ev_fork = nullptr, ev_join = nullptr;
  hipStream_t prep_stream = nullptr; hipEvent_t ev_hashed[MUL_NBUF] = {};  // `mul -raw`: the lines are hashed on a stream of their own, ahead of the pieces
  devbuf<u32> d_list; u64 list_n = 0;          // optional sorted hash list (exact confirm on the device)
  devbuf<ecl_found_dev> d_found;
  devbuf<u32> d_counter; pinbuf<u32> pin_counter;  // the words of callstate.h (the page-locked host copy: read back by the copy engine, no compute slot needed)
  // key coverage (ecl_hip_get_coverage): keys / scalars of the calls that launched or were served from a sweep, those of them whose device
  // count matched, and the keys the kernels of this context's launches counted; never reset
  uint64_t cov_requested = 0, cov_covered = 0, cov_device = 0;
  bool diag_drop = false;  // ecl_hip_diag_drop_round: the next search launch runs one round short
  last_records last;  // where the records of the last add_range / mul_batch call are (ecl_hip_fetch_found; callstate.h)
  // walk state for contiguous continuation
  bool walk_valid = false;
  u32 walk_T = 0, walk_B = 0;
  bool B_auto = true;  // half group not fixed by the caller: short calls take a smaller one (see ecl_hip_add_range)
  u256 walk_next;  // scalar (mod n) the resident centres are positioned for
  u32 jump_host[16];
  u32 aux_B = 0, aux_T = 0;  // geometry the jump and the ladder in d_aux / jump_host were computed for
  // ECL_ORIGIN: the origin point of the call in hand (canonical words x[8], y[8]; set by ecl_hip_add_range) and the one the resident
  // walk was positioned with: a call continues the walk only if they are equal
  u32 origin_w[16] = {}, walk_origin[16] = {};
  // ECL_HERD: the resident herd (22 words per kangaroo), its jump table, and the sixteen limbs it was built from: a call continues the
  // herd only if its block equals them
  devbuf<u32> d_herd, d_herdtab;
  uint64_t herd_blk[16] = {}; bool herd_valid = false;
  LA_CONTEXT_MEMBERS
  // timing
  double kernel_ms = 0, setup_ms = 0, mul_ms = 0;
  uint64_t launches = 0, keys = 0, setups = 0, mul_calls = 0, mul_scalars = 0;
  hipEvent_t ev_s0 = nullptr, ev_s1 = nullptr;
};

#define HIPCHK(h, call)                                                                    \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) {                                                                \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
      return ECL_E_HIP;                                                                    \
    }                                                                                      \
  } while (0)


static void release_multable(struct ecl_hip* h);
static void la_leave(struct ecl_hip* h);
static void la_filter_changed(struct ecl_hip* h, const uint64_t* bits, uint64_t nwords);
static void la_list_changed(struct ecl_hip* h, const uint32_t (*h160)[5], uint64_t n);
static u64 la_default_max();

static void words_of(u32 w[8], const u256& a) {
  for (int i = 0; i < 4; ++i) w[2 * i] = (u32)a.w[i], w[2 * i + 1] = (u32)(a.w[i] >> 32);
}

extern "C" {

int ecl_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* ecl_hip_strerror(int code) {
  switch (code) {
  case ECL_OK: return "ok";
  case ECL_E_ARG: return "bad argument";
  case ECL_E_HIP: return "HIP runtime error";
  case ECL_E_NODEV: return "no such GPU";
  case ECL_E_OVERFLOW: return "more hits than the output buffer holds";
  case ECL_E_NOBLOOM: return "no bloom filter set";
  case ECL_E_RANGE: return "range touches scalar 0 (mod n)";
  case ECL_E_SELFTEST: return "device self-test failed";
  case ECL_E_COVERAGE: return "the device did not hash every key of the call";
  default: return "unknown error";
  }
}
const char* ecl_hip_last_error(const ecl_hip* h) { return h ? h->err.c_str() : ""; }

int ecl_hip_open(ecl_hip** out, int device, uint32_t flags, uint32_t ord_offs) {
  const u32 types = ECL_ADDR33 | ECL_ADDR65 | ECL_P2SH;
  // the hash of `mul -raw` (ECL_KDF_*): beside every context that has a `mul`; it is kept apart from the other flags, which are then
  // checked, and later read, as on a context without it
  const u32 kdf = flags & ECL_KDF_CAMP2;
  if (kdf && (flags & (ECL_ORIGIN | ECL_INSERT | ECL_HERD | ECL_PREFIX | ECL_MASK))) return ECL_E_ARG;
  flags &= ~ECL_KDF_CAMP2;
  // BIP39 phrases in place of hashed lines (ECL_KDF_BIP39): beside the same contexts, and not beside an ECL_KDF_* bit
  const u32 bip39 = flags & ECL_KDF_BIP39;
  if (bip39 && (kdf || (flags & (ECL_ORIGIN | ECL_INSERT | ECL_HERD | ECL_PREFIX | ECL_MASK)))) return ECL_E_ARG;
  flags &= ~ECL_KDF_BIP39;
  // lines generated on the device from a template (ECL_GEN): beside the same contexts, with or without an ECL_KDF_* bit, not beside ECL_KDF_BIP39
  const u32 gen = flags & ECL_GEN;
  if (gen && (bip39 || (flags & (ECL_ORIGIN | ECL_INSERT | ECL_HERD | ECL_PREFIX | ECL_MASK)))) return ECL_E_ARG;
  flags &= ~ECL_GEN;
  if (!out || ord_offs > 255 || !(flags & (types | ECL_ETH | ECL_TR | ECL_PUB)) ||
      (flags & ~(types | ECL_ETH | ECL_TR | ECL_PUB | ECL_ENDO | ECL_ORIGIN | ECL_INSERT | ECL_HERD | ECL_PREFIX | ECL_MASK)))
    return ECL_E_ARG;
  // the mask filter: beside eth alone, with or without the endomorphism and, for a split-key search, from an origin
  if ((flags & ECL_MASK) && (!(flags & ECL_ETH) || (flags & ~(ECL_MASK | ECL_ETH | ECL_ENDO | ECL_ORIGIN)))) return ECL_E_ARG;
  // the prefix filter: beside addr33 / addr65 or beside eth, with or without the endomorphism
  // (and, for a split-key search, from an origin: ECL_PREFIX | ECL_ORIGIN beside the same types)
  if ((flags & ECL_PREFIX) && (flags & ~(ECL_PREFIX | ECL_ORIGIN | ECL_ADDR33 | ECL_ADDR65 | ECL_ETH | ECL_ENDO))) return ECL_E_ARG;
  // the two walks of `bsgs`: each valid only as ECL_PUB | ECL_ORIGIN / ECL_PUB | ECL_INSERT (no endomorphism, no other type, not both);
  // the origin of a hashing walk only on a prefix or a mask context
  if ((flags & ECL_ORIGIN) && !(flags & (ECL_PREFIX | ECL_MASK)) && flags != (ECL_PUB | ECL_ORIGIN)) return ECL_E_ARG;
  if ((flags & ECL_INSERT) && flags != (ECL_PUB | ECL_INSERT)) return ECL_E_ARG;
  // the herd of `kangaroo`: valid only as ECL_PUB | ECL_HERD; ord_offs is the number of distinguished-point bits
  if ((flags & ECL_HERD) && (flags != (ECL_PUB | ECL_HERD) || ord_offs > 32)) return ECL_E_ARG;
  if ((flags & ECL_ETH) && (flags & types)) return ECL_E_ARG;  // eth is searched alone
  if ((flags & ECL_TR) && flags != ECL_TR) return ECL_E_ARG;   // Taproot is searched alone and without the endomorphism
  if ((flags & ECL_PUB) && (flags & ~(ECL_PUB | ECL_ENDO | ECL_ORIGIN | ECL_INSERT | ECL_HERD))) return ECL_E_ARG;  // public keys are searched alone
  int n = ecl_hip_device_count();
  if (device < 0 || device >= n) return ECL_E_NODEV;
  ecl_hip* h = new ecl_hip();
  h->dev = device, h->flags = flags, h->kdf = kdf, h->bip39 = bip39 != 0, h->gen = gen != 0, h->offs = ord_offs, h->la_max = la_default_max();
  *out = h;
  HIPCHK(h, hipSetDevice(device));
  HIPCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  HIPCHK(h, hipEventCreate(&h->ev0));
  HIPCHK(h, hipEventCreate(&h->ev1));
  HIPCHK(h, hipEventCreate(&h->ev_s0));
  HIPCHK(h, hipEventCreate(&h->ev_s1));
  HIPCHK(h, h->d_aux.grow(ECL_AUX_WORDS + 1));
  HIPCHK(h, h->d_auxk.grow(34 * 8));
  HIPCHK(h, h->d_counter.grow(CW_DEVICE_WORDS));
  HIPCHK(h, h->pin_counter.grow(CW_HOST_WORDS));
  h->pin_counter.p[CW_ORIGIN_INF] = 0;
  // the self-test checks the CODE (known answers, walk kernel against the double-and-add kernel): once per process
  // for every (device, kernel selection) is enough - eight handles for eight shards of one scan do not repeat it
  static std::mutex mu;
  static std::set<u64> passed;
  const char* skip = getenv("ECL_HIP_SKIP_SELFTEST");
  const u64 key = (u64)device << 32 | (flags | kdf | bip39 | gen);  // (every bit of ecl_hip_open's flags: no two kernel selections share a record)
  {
    std::lock_guard<std::mutex> lk(mu);
    if ((skip && skip[0] == '1') || passed.count(key)) return ECL_OK;
  }
  const int rc = ecl_hip_selftest(h);
  if (rc == ECL_OK) {
    std::lock_guard<std::mutex> lk(mu);
    passed.insert(key);
  }
  return rc;
}

void ecl_hip_close(ecl_hip* h) {
  if (!h) return;
  la_leave(h);
  (void)hipSetDevice(h->dev);
  // no buffer is freed before every stream of the context has been waited for: the buffers are the context's members and go with it, last
  for (hipStream_t st : {h->stream, h->stream2, h->copy_stream, h->prep_stream})
    if (st) (void)hipStreamSynchronize(st);
  release_multable(h);
  for (int i = 0; i < MUL_NBUF; ++i)
    for (hipEvent_t ev : {h->ev_copied[i], h->ev_free[i], h->ev_hashed[i]})
      if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : {h->ev_fork, h->ev_join, h->ev_s0, h->ev_s1, h->ev0, h->ev1})
    if (ev) (void)hipEventDestroy(ev);
  for (hipStream_t st : {h->copy_stream, h->stream2, h->prep_stream, h->stream})
    if (st) (void)hipStreamDestroy(st);
  delete h;
}

}  // extern "C"
// ECL_PREFIX: the filter words are the range table (ten 32-bit words per range); the stage-1 bitmap is built here and goes to the device
// in front of it, in one allocation
#define PREFIX_BITMAP_WORDS64 ((((u64)1 << PREFIX_BUCKET_BITS) / 64u))
static prefix_t prefix_of(const ecl_hip* h) {
  prefix_t p;
  p.bitmap = (const u32*)h->d_bloom.p, p.table = (const u32*)(h->d_bloom.p + PREFIX_BITMAP_WORDS64);
  p.n = h->prefix_n, p.shift = 32u - PREFIX_BUCKET_BITS;
  return p;
}
static int prefix_set_table(ecl_hip* h, const u32* table, uint64_t nwords) {
  if (nwords % 5 != 0 || !prefix_table_ok(table, nwords / 5)) {
    h->err = "ecl_hip_set_bloom: a prefix table is 1 ... 65536 ranges lo[5], hi[5] with lo <= hi, sorted and disjoint";
    return ECL_E_ARG;
  }
  const u32 n = (u32)(nwords / 5);
  HIPCHK(h, hipSetDevice(h->dev));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->d_bloom.reset(), h->bloom_words = 0, h->prefix_n = 0;  // (a filter is as large as it is: never kept for a smaller one)
  std::vector<u64> img(PREFIX_BITMAP_WORDS64 + nwords);
  prefix_build_bitmap((u32*)img.data(), table, n, 32u - PREFIX_BUCKET_BITS);
  memcpy(img.data() + PREFIX_BITMAP_WORDS64, table, (size_t)nwords * sizeof(u64));
  HIPCHK(h, h->d_bloom.grow(img.size()));
  HIPCHK(h, hipMemcpyAsync(h->d_bloom.p, img.data(), img.size() * sizeof(u64), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->bloom_words = img.size(), h->prefix_n = n;
  return ECL_OK;
}
// ECL_MASK: the filter words are the mask table (ten 32-bit words per entry) and go to the device as they are.  A refused table leaves the
// context with none
static mask_t mask_of(const ecl_hip* h) {
  mask_t m;
  memset(&m, 0, sizeof m);
  m.table = (const u32*)h->d_bloom.p, m.n = h->mask_n;
  return m;
}
static int mask_set_table(ecl_hip* h, const u32* table, uint64_t nwords) {
  HIPCHK(h, hipSetDevice(h->dev));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->d_bloom.reset(), h->bloom_words = 0, h->mask_n = 0;
  if (nwords % 5 != 0 || !mask_table_ok(table, nwords / 5)) {
    h->err = "ecl_hip_set_bloom: a mask table is 1 ... 16 entries m[5], v[5] with no bit of v outside m and no entry twice";
    return ECL_E_ARG;
  }
  HIPCHK(h, h->d_bloom.grow(nwords));
  HIPCHK(h, hipMemcpyAsync(h->d_bloom.p, table, nwords * sizeof(u64), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->bloom_words = nwords, h->mask_n = (u32)(nwords / 5);
  return ECL_OK;
}
extern "C" {
int ecl_hip_set_bloom(ecl_hip* h, const uint64_t* bits, uint64_t nwords) {
  if (!h || !bits || nwords == 0 || nwords >= (1ull << 58)) return ECL_E_ARG;
  if (h->flags & ECL_PREFIX) return prefix_set_table(h, (const u32*)bits, nwords);
  if (h->flags & ECL_MASK) return mask_set_table(h, (const u32*)bits, nwords);
  HIPCHK(h, hipSetDevice(h->dev));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  la_leave(h), h->la_key_valid = false;
  h->d_bloom.reset(), h->bloom_words = 0;
  HIPCHK(h, h->d_bloom.grow(nwords));
  // on the handle's own stream: device threads upload in parallel, each over its own PCIe link; memory from ecl_hip_alloc_host goes
  // by DMA at link rate, a pageable buffer is staged by the runtime
  HIPCHK(h, hipMemcpyAsync(h->d_bloom.p, bits, nwords * sizeof(u64), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->bloom_words = nwords;
  la_filter_changed(h, bits, nwords);
  return ECL_OK;
}

// Page-locked host memory comes from the runtime (hipHostMalloc, next to the GPU's NUMA node), never from registering the caller's
// own memory in place: hipHostRegister / hipHostUnregister cycles on memory that the host allocator recycles end in GPU memory access
// faults inside the ROCm runtime (rounds 2 and 5; profiles/r05_pin_fault.txt), which is why the entry points
// that used to do that are gone.  Pageable buffers are copied by the runtime (filter) or staged through the library's own pinned
// buffers (scalar arrays of ecl_hip_mul_batch).
#define ECL_PIN_MIN_BYTES ((size_t)1 << 20)  /* ecl_hip_mul_batch: batches below this are staged whatever their memory is */
void* ecl_hip_alloc_host(size_t bytes) {
  void* p = nullptr;
  if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) return nullptr;
  return p;
}
void ecl_hip_free_host(void* p) {
  if (p) (void)hipHostFree(p);
}

int ecl_hip_set_list(ecl_hip* h, const uint32_t (*h160)[5], uint64_t n) {
  if (!h || (n && !h160) || (h->flags & (ECL_PREFIX | ECL_MASK))) return ECL_E_ARG;
  for (uint64_t i = 1; i < n; ++i) {  // strictly increasing in compare_160 order (addr.c:18-26)
    int c = 0;
    for (int k = 0; k < 5 && c == 0; ++k) c = h160[i - 1][k] < h160[i][k] ? -1 : (h160[i - 1][k] > h160[i][k] ? 1 : 0);
    if (c >= 0) {
      h->err = "ecl_hip_set_list: the list is not sorted and unique";
      return ECL_E_ARG;
    }
  }
  HIPCHK(h, hipSetDevice(h->dev));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  la_leave(h);
  h->d_list.reset(), h->list_n = 0;
  la_list_changed(h, h160, 0);
  if (n == 0) return ECL_OK;
  HIPCHK(h, h->d_list.grow(n * 5));
  HIPCHK(h, hipMemcpy(h->d_list.p, h160, n * 20, hipMemcpyHostToDevice));
  h->list_n = n;
  la_list_changed(h, h160, n);
  return ECL_OK;
}

// ---- load_filter's list preparation (main.c:96-131: qsort by compare_160, then one blf_add per entry) on the device ------
// 10^7 entries cost the host 13 s (qsort of 20-byte records + 2 * 10^8 scattered bit sets), 10^8 two minutes; here: five
// stable 32-bit radix sorts of a permutation (least significant word first = compare_160's word-by-word order,
// addr.c:18-26; each four 8-bit passes: aux_kernels.h), a gather, adjacent-duplicate flags + exclusive scan + scatter.  The bits are
// set by the bulk insert kernel into a filter of the reference's list-mode size (2 words per entry).
}  // extern "C"
// exclusive scan of n counts on the handle's stream; `tmp` holds the two upper levels (n / 2048 + n / 2048^2 + 2 words)
static u64 scan_tmp_words(u64 n) {
  const u64 per = (u64)SCAN_BLOCK * SCAN_PER, l1 = (n + per - 1) / per, l2 = (l1 + per - 1) / per;
  return l1 + l2 + 2;
}
static int scan_exclusive(ecl_hip* h, const u32* in, u32* out, u64 n, u32* tmp) {
  const u64 per = (u64)SCAN_BLOCK * SCAN_PER, nb = (n + per - 1) / per;
  if (nb <= 1) {
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(SCAN_BLOCK), 0, h->stream, in, out, n, (u32*)nullptr);
    HIPCHK(h, hipGetLastError());
    return ECL_OK;
  }
  hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, h->stream, in, out, n, tmp);
  HIPCHK(h, hipGetLastError());
  const int rc = scan_exclusive(h, tmp, tmp, nb, tmp + nb);  // the workgroups' totals, in place, one level up
  if (rc != ECL_OK) return rc;
  hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nb), dim3(SCAN_BLOCK), 0, h->stream, out, n, tmp);
  HIPCHK(h, hipGetLastError());
  return ECL_OK;
}
// stable sort of the n (key, value) pairs by key: four 8-bit passes, result back in key[0] / val[0]
static int rsort_pairs(ecl_hip* h, u32* key[2], u32* val[2], u32 n, u32 nt, u32 L, u32* counts, u32* scan_tmp) {
  const dim3 grid((nt + RSORT_BLOCK - 1) / RSORT_BLOCK), blk(RSORT_BLOCK);
  int cur = 0;
  for (u32 shift = 0; shift < 32; shift += 8) {
    hipLaunchKernelGGL(k_rsort_count, grid, blk, 0, h->stream, key[cur], n, nt, L, shift, counts);
    HIPCHK(h, hipGetLastError());
    const int rc = scan_exclusive(h, counts, counts, (u64)256 * nt, scan_tmp);
    if (rc != ECL_OK) return rc;
    hipLaunchKernelGGL(k_rsort_scatter, grid, blk, 0, h->stream, key[cur], val[cur], n, nt, L, shift, counts, key[cur ^ 1], val[cur ^ 1]);
    HIPCHK(h, hipGetLastError());
    cur ^= 1;
  }
  return ECL_OK;  // four passes: an even number of swaps
}
extern "C" {
int ecl_hip_sort_list(ecl_hip* h, uint32_t (*h160)[5], uint64_t n, uint64_t* kept) {
  if (!h || !kept || (n && !h160) || n >= (1ull << 31)) return ECL_E_ARG;
  *kept = 0;
  if (n == 0) return ECL_OK;
  HIPCHK(h, hipSetDevice(h->dev));
  const u32 N = (u32)n;
  // threads of the sort: tiles of at least 256 elements, at most 65536 threads
  u32 nt = (N + 255u) / 256u;
  nt = nt < RSORT_BLOCK ? RSORT_BLOCK : nt > 65536u ? 65536u : nt;
  const u32 L = (N + nt - 1) / nt;
  devbuf<u32> rec, out, key[2], perm[2], flag, pos, counts, tmp;
  HIPCHK(h, rec.grow((size_t)N * 5));
  HIPCHK(h, out.grow((size_t)N * 5));
  for (int i = 0; i < 2; ++i) {
    HIPCHK(h, key[i].grow(N));
    HIPCHK(h, perm[i].grow(N));
  }
  HIPCHK(h, flag.grow(N));
  HIPCHK(h, pos.grow(N));
  HIPCHK(h, counts.grow((size_t)256 * nt));
  const u64 tmp_words = scan_tmp_words((u64)256 * nt) > scan_tmp_words(N) ? scan_tmp_words((u64)256 * nt) : scan_tmp_words(N);
  HIPCHK(h, tmp.grow((size_t)tmp_words));
  HIPCHK(h, hipMemcpyAsync(rec.p, h160, (size_t)N * 20, hipMemcpyHostToDevice, h->stream));
  const dim3 grid((N + 255) / 256), blk(256);
  hipLaunchKernelGGL(k_list_iota, grid, blk, 0, h->stream, perm[0].p, N);
  u32* kk[2] = {key[0].p, key[1].p};
  u32* pp[2] = {perm[0].p, perm[1].p};
  for (int word = 4; word >= 0; --word) {  // LSD: the last word first, every sort stable
    hipLaunchKernelGGL(k_list_key, grid, blk, 0, h->stream, rec.p, pp[0], kk[0], N, (u32)word);
    HIPCHK(h, hipGetLastError());
    const int rc = rsort_pairs(h, kk, pp, N, nt, L, counts.p, tmp.p);
    if (rc != ECL_OK) return rc;
  }
  hipLaunchKernelGGL(k_list_gather_flag, grid, blk, 0, h->stream, rec.p, pp[0], out.p, flag.p, N);
  HIPCHK(h, hipGetLastError());
  {
    const int rc = scan_exclusive(h, flag.p, pos.p, N, tmp.p);
    if (rc != ECL_OK) return rc;
  }
  hipLaunchKernelGGL(k_list_compact, grid, blk, 0, h->stream, out.p, flag.p, pos.p, rec.p, N);
  HIPCHK(h, hipGetLastError());
  u32 last_pos = 0, last_flag = 0;
  HIPCHK(h, hipMemcpyAsync(&last_pos, pos.p + (N - 1), 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&last_flag, flag.p + (N - 1), 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const u64 k = (u64)last_pos + last_flag;
  HIPCHK(h, hipMemcpy(h160, rec.p, (size_t)k * 20, hipMemcpyDeviceToHost));
  *kept = k;
  return ECL_OK;
}

int ecl_hip_set_geometry(ecl_hip* h, uint32_t half_group, uint32_t max_lanes) {
  if (!h) return ECL_E_ARG;
  if (half_group) {
    if (half_group < 2 || half_group > (1u << 16)) return ECL_E_ARG;
    h->B = half_group, h->B_auto = false;
  }
  if (max_lanes) h->Tmax = (max_lanes + 255u) & ~255u;
  if (half_group || max_lanes) h->geom_fixed = true, la_leave(h);
  h->walk_valid = false;
  return ECL_OK;
}

int ecl_hip_get_timing(ecl_hip* h, double* kernel_ms, uint64_t* launches, uint64_t* keys) {
  if (!h) return ECL_E_ARG;
  if (kernel_ms) *kernel_ms = h->kernel_ms;
  if (launches) *launches = h->launches;
  if (keys) *keys = h->keys;
  return ECL_OK;
}
int ecl_hip_get_coverage(ecl_hip* h, uint64_t* requested, uint64_t* covered, uint64_t* device_keys) {
  if (!h) return ECL_E_ARG;
  if (requested) *requested = h->cov_requested;
  if (covered) *covered = h->cov_covered;
  if (device_keys) *device_keys = h->cov_device;
  return ECL_OK;
}
int ecl_hip_reset_timing(ecl_hip* h) {
  if (!h) return ECL_E_ARG;
  h->kernel_ms = 0, h->launches = 0, h->keys = 0, h->setup_ms = 0, h->setups = 0;
  h->mul_ms = 0, h->mul_calls = 0, h->mul_scalars = 0;
  return ECL_OK;
}
int ecl_hip_get_setup_timing(ecl_hip* h, double* setup_ms, uint64_t* setups) {
  if (!h) return ECL_E_ARG;
  if (setup_ms) *setup_ms = h->setup_ms;
  if (setups) *setups = h->setups;
  return ECL_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ add path (host)

typedef void (*add_kernel_t)(const add_args);
// every non-empty set of address types (ecl_hip_open refuses the empty one) x endo
static add_kernel_t pick_add_kernel(u32 flags) {
  const bool endo = flags & ECL_ENDO;
  if (flags & ECL_MASK) return endo ? k_add_msk_eth<true> : k_add_msk_eth<false>;  // beside eth alone (ecl_hip_open): the mask filter
  if (flags & ECL_PREFIX) {  // beside addr33 / addr65 or eth (ecl_hip_open): the prefix filter in place of the bloom
    if (flags & ECL_ETH) return endo ? k_add_pfx_eth<true> : k_add_pfx_eth<false>;
    switch (flags & (ECL_ADDR33 | ECL_ADDR65)) {
    case ECL_ADDR33: return endo ? k_add_pfx<true, false, true> : k_add_pfx<true, false, false>;
    case ECL_ADDR65: return endo ? k_add_pfx<false, true, true> : k_add_pfx<false, true, false>;
    default: return endo ? k_add_pfx<true, true, true> : k_add_pfx<true, true, false>;
    }
  }
  if (flags & ECL_INSERT) return k_add_pub_ins;  // ECL_PUB | ECL_INSERT alone (ecl_hip_open): sets filter bits, no records
  if (flags & ECL_PUB) return endo ? k_add_pub<true> : k_add_pub<false>;  // alone (ecl_hip_open)
  if (flags & ECL_TR) return k_add_tr;  // alone, no endomorphism (ecl_hip_open): the emit kernel
  if (flags & ECL_ETH) return endo ? k_add_eth<true> : k_add_eth<false>;  // alone (ecl_hip_open)
  switch (flags & (ECL_ADDR33 | ECL_ADDR65 | ECL_P2SH)) {
  case ECL_ADDR33: return endo ? k_add<true, false, true> : k_add<true, false, false>;
  case ECL_ADDR65: return endo ? k_add<false, true, true> : k_add<false, true, false>;
  case ECL_ADDR33 | ECL_ADDR65: return endo ? k_add<true, true, true> : k_add<true, true, false>;
  case ECL_P2SH: return endo ? k_add_p2sh<false, false, true> : k_add_p2sh<false, false, false>;
  case ECL_ADDR33 | ECL_P2SH: return endo ? k_add_p2sh<true, false, true> : k_add_p2sh<true, false, false>;
  case ECL_ADDR65 | ECL_P2SH: return endo ? k_add_p2sh<false, true, true> : k_add_p2sh<false, true, false>;
  default: return endo ? k_add_p2sh<true, true, true> : k_add_p2sh<true, true, false>;
  }
}

// found records of one call: [0, rcap) written by the search kernel; in list mode the confirmed ones are compacted into
// [rcap, 2 * rcap).  rcap = max(cap, 2^20) whatever the caller's `cap` (32 MB of HBM, twice that in list mode): a call that reports
// ECL_E_OVERFLOW has kept the records that did not fit the caller's buffer, and ecl_hip_fetch_found hands them over without the search
// kernel running again.
#define ECL_RAW_CAP_MIN (1u << 20)
#define ECL_CAP_MAX (1u << 30)  /* records one call can be asked to deliver (32 GB of them); list mode allocates twice the count */
static u32 raw_cap_of(u32 cap) { return cap > ECL_RAW_CAP_MIN ? cap : ECL_RAW_CAP_MIN; }
// the record buffer of a call that keeps rcap records (rcap <= 2^30): the one sizing rule
static int ensure_found(ecl_hip* h, u32 rcap) {
  const size_t want = h->d_list.p ? 2 * (size_t)rcap : rcap;
  if (want <= h->d_found.n) return ECL_OK;
  if (!h->last.from_host) h->last.forget();  // the buffer that held the last call's records goes away (records on the host stay)
  HIPCHK(h, h->d_found.grow(want));
  return ECL_OK;
}
static int fetch_records(ecl_hip* h, ecl_found* out, u32 from, u32 n, bool keep_endo) {
  if (!n) return ECL_OK;
  std::vector<ecl_found_dev> tmp(n);
  HIPCHK(h, hipMemcpy(tmp.data(), h->d_found.p + from, (size_t)n * sizeof(ecl_found_dev), hipMemcpyDeviceToHost));
  for (u32 i = 0; i < n; ++i) {
    out[i].key_offset = tmp[i].key_offset;
    memcpy(out[i].h160, tmp[i].h160, 20);
    out[i].endo = keep_endo ? (uint8_t)(tmp[i].tag & 0xff) : 0, out[i].compressed = (uint8_t)((tmp[i].tag >> 8) & 0xff);
    out[i].pad[0] = out[i].pad[1] = 0;
  }
  return ECL_OK;
}

// The frame of a search call - add_core, tr_add_core, herd_add_core, ecl_hip_mul_batch, ecl_hip_mul_batch_raw: begin(), args() for the
// kernels, reset() in front of the launches (once per pass of -raw), collect() behind them, finish().  What a call decides from the words
// read back is call_verdict_of (callstate.h); here are the HIP calls around it and the books.
// Key coverage: every launch of a search kernel counts, on the device, the keys that reach the hash-and-probe step inside its range
// (add_kernel.h: keys_count / keys_flush) into the u64 at CW_KEYS.  A call whose count differs from the keys it asked for returns
// ECL_E_COVERAGE: no records, nothing to fetch, and the resident walk is dropped.
struct call_frame {
  ecl_hip* h;
  const char* what;   // the call's name in the text of a short count
  const char* what2;  // null, or: the second count (CW_TR_CHECKED) is checked too, under this name
  u64 n;              // keys / scalars asked for
  ecl_found* out;
  u32 cap;
  u32* nout;
  bool mul, endo;     // booked as a `mul` call; the records' endo byte is meaningful
  u32 rcap = 0;
  call_verdict v = {};

  // the records of the call before are about to be overwritten
  int begin() {
    h->last.forget();
    rcap = raw_cap_of(cap);
    return ensure_found(h, rcap);
  }
  // the common half of a search kernel's arguments: filter, record buffer, counters, the word its keys are counted into
  add_args args(u32 keys_at = CW_KEYS) const {
    add_args a;
    memset(&a, 0, sizeof a);
    a.bloom = bloom_make(h->d_bloom.p, h->bloom_words);
    a.found = h->d_found.p, a.counter = h->d_counter.p, a.cap = rcap, a.keys = (unsigned long long*)(h->d_counter.p + keys_at);
    return a;
  }
  int reset() const {
    HIPCHK(h, hipMemsetAsync(h->d_counter.p, 0, CW_DEVICE_WORDS * sizeof(u32), h->stream));
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    return ECL_OK;
  }
  // after the search kernels have been queued on h->stream: optional list confirm, then counters and records to the host
  int collect() {
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    const bool lst = h->d_list.p != nullptr;
    if (lst) {
      const u32 blocks = (rcap + 255) / 256 < 1024 ? (rcap + 255) / 256 : 1024;
      hipLaunchKernelGGL(k_list_filter, dim3(blocks), dim3(256), 0, h->stream, h->d_found.p, h->d_counter.p + CW_PUSHED, rcap, h->d_list.p, h->list_n,
                         h->d_found.p + rcap, h->d_counter.p + CW_CONFIRMED, rcap);
      HIPCHK(h, hipGetLastError());
    }
    // One read-back and one wait per call, into page-locked memory: a copy into pageable memory goes through a staging kernel, and with
    // a second context's k_mul_check launches filling the chip every small kernel waits milliseconds for a slot (each such wait at the
    // end of a `mul` call is time this context has nothing in flight).  All the words: the records, the flags and both counts.
    const u32* w = h->pin_counter.p;
    HIPCHK(h, hipMemcpyAsync(h->pin_counter.p, h->d_counter.p, CW_DEVICE_WORDS * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    v = call_verdict_of(w, cap, rcap, lst, n, what2 ? &n : nullptr);
    h->cov_device += counted_keys(w);
    h->last.on_device(v.from, v.held, v.total, endo);
    return fetch_records(h, out, v.from, v.take, endo);
  }
  // the books (a short call was launched: it is booked too), the verdict's text and state, *nout -> the call's result
  int finish(u32 launches = 1, u32 setups = 0) {
    float ms = 0;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));  // copies + kernels of this call, as the stream saw them
    if (mul) h->mul_ms += ms, h->mul_calls += 1, h->mul_scalars += n;
    else h->kernel_ms += ms, h->launches += launches, h->keys += n;
    if (setups) {  // (the events hold the last set-up of the call)
      HIPCHK(h, hipEventElapsedTime(&ms, h->ev_s0, h->ev_s1));
      h->setup_ms += ms * setups, h->setups += setups;
    }
    char msg[160];
    if (call_verdict_text(v, what, what2, n, msg, sizeof msg)) h->err = msg;
    if (v.rc == ECL_E_COVERAGE) h->walk_valid = false, h->last.forget();
    *nout = v.nout;
    return v.rc;
  }
  // a refusal behind finish(): no records, nothing to fetch
  int refuse(int rc, const char* why) {
    h->err = why, h->last.forget(), *nout = 0;
    return rc;
  }
};
static int count_call(ecl_hip* h, u64 n, int rc) {  // the totals of ecl_hip_get_coverage for one add / mul call, by its result
  if (rc_was_launched(rc)) h->cov_requested += n;
  if (rc_was_whole(rc)) h->cov_covered += n;
  return rc;
}

static int la_fetch(ecl_hip* h, uint32_t first, ecl_found* out, uint32_t n, uint32_t* got);
extern "C" int ecl_hip_fetch_found(ecl_hip* h, uint32_t first, ecl_found* out, uint32_t n, uint32_t* got) {
  if (!h || !got || (!out && n)) return ECL_E_ARG;
  *got = 0;
  if (h->last.from_host) return la_fetch(h, first, out, n, got);  // the last call was served from a look-ahead sweep: its records are on the host
  if (first >= h->last.held || n == 0) return ECL_OK;
  const u32 take = h->last.held - first < n ? h->last.held - first : n;
  HIPCHK(h, hipSetDevice(h->dev));
  const int rc = fetch_records(h, out, h->last.at + first, take, h->last.endo);
  if (rc == ECL_OK) *got = take;
  return rc;
}

static int default_lanes(ecl_hip* h) {
  if (h->Tmax) return ECL_OK;
  hipDeviceProp_t p;
  HIPCHK(h, hipGetDeviceProperties(&p, h->dev));
  int occ = 0;
  HIPCHK(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)pick_add_kernel(h->flags), ECL_ADD_BLOCK, 0));
  if (occ < 1) occ = 1;
  const u32 resident = (u32)p.multiProcessorCount * (u32)occ * (u32)ECL_ADD_BLOCK;
  // Oversubscribe: with exactly the resident number of lanes every wave of the chip is in the same phase at the same
  // time (prefix products, then the inversion chain, then the hash-heavy walk back); with several times more blocks
  // than slots the dispatcher staggers them and the phases overlap.  Measured on addr33: 196608 lanes (resident)
  // 10.9 Gkeys/s, 786432 11.5, 1048576 12.0, 2097152 12.1 (final kernel: 12.49 / 12.63 at 2^20 / 2^21, no more
  // beyond).  The chains cost lanes * B * 36 bytes of HBM (2^21 lanes, B = 1024: 77 GB of the 288), so the factor is
  // cut back if memory is short.
  u64 lanes = 1ull << 21;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
    while (lanes > resident && lanes * h->B * 36ull > free_b / 3) lanes /= 2;
  }
  if (lanes < resident) lanes = resident;
  h->Tmax = (u32)((lanes + 255) & ~255ull);
  return ECL_OK;
}

// table of (i+1)*stride*G, i < B (ctx_precompute_gpoints, main.c:219-246: only x,y of the positive half are stored)
static int ensure_table(ecl_hip* h) {
  if (h->d_tab.p && h->tab_B == h->B) return ECL_OK;
  h->d_tab.reset(), h->tab_B = 0;  // (a table is as large as its half group)
  const u32 B = h->B;
  std::vector<u32> ks((size_t)B * 8);
  u256 s = sc_pow2(h->offs), cur = s;
  for (u32 i = 0; i < B; ++i) {
    words_of(&ks[(size_t)i * 8], cur);
    cur = sc_add(cur, s);
  }
  devbuf<u32> d_k, d_w;  // freed on every way out
  HIPCHK(h, d_k.grow(ks.size()));
  HIPCHK(h, d_w.grow((size_t)B * 16));
  HIPCHK(h, h->d_tab.grow((size_t)B * ECL_TAB_STRIDE));
  HIPCHK(h, hipMemcpyAsync(d_k.p, ks.data(), ks.size() * sizeof(u32), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_mul_g, dim3((B + 63) / 64), dim3(64), 0, h->stream, d_k.p, d_w.p, (u8*)nullptr, B);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_tab_to_limbs, dim3((B + 63) / 64), dim3(64), 0, h->stream, d_w.p, h->d_tab.p, B);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->tab_B = B;
  return ECL_OK;
}

extern "C" int ecl_hip_get_geometry(ecl_hip* h, uint32_t* half_group, uint32_t* lanes) {
  if (!h) return ECL_E_ARG;
  HIPCHK(h, hipSetDevice(h->dev));
  int rc = default_lanes(h);
  if (rc != ECL_OK) return rc;
  if (half_group) *half_group = h->B;
  if (lanes) *lanes = h->Tmax;
  return ECL_OK;
}

// Geometry of one call.  The table for half group h->B holds the tables of all smaller ones as prefixes, so a call may walk any
// power-of-two half group up to h->B.  Two costs pull in opposite directions: a lane pays one inversion per group (the division
// steps cost about five keys' worth of work: + 5 / 2B per key; inv_keys_worth: a public key costs a fraction of a hashed one, so the same
// inversion is worth several times as many of them), and a walk with few lanes leaves the chip empty or in lock-step -
// the kernel only reaches its rate when the slots are oversubscribed with blocks in different phases.  Both were measured
// (profiles/r05_short_calls.txt: calls of 2^21 ... 2^26 keys at half groups 8 ... 128; profiles/r04_short_calls.txt: 2^29 ... 2^32):
// the time per key relative to the long-call rate is, to a few per cent, lane_factor(lanes) x (1 + 5 / 2B) with
//   lanes        2^13  2^14  2^15  2^16  2^17  2^18  2^19  2^20  2^21
//   lane_factor  10.9   5.5  2.77  1.41  1.17  1.10  1.04  1.00  0.975
// and the automatic choice is the half group that minimises the product.  That gives 1024 x 2^21 lanes for 2^32 keys, 128 x 2^21 for
// 2^29 (the per-GPU shard of the named range on 8 GPUs; as round 4 found by sweeping), 32 x 2^18 for 2^24 and 8 x 2^17 for the
// reference's own MAX_JOB_SIZE of 2^21 keys (main.c:16) - 7.1 Gkeys/s where the round-4 floor of 128 (8192 lanes: 32 workgroups on
// 256 CUs) gave 1.1.  Contiguous calls of one size keep one geometry, so they still continue the resident walk.
#define ECL_B_FLOOR 8u  /* k_init_centres_batched parks 144 bytes per lane in the chain scratch (lanes * B * 36 bytes) */
static double lane_factor(double lanes) {
  static const double f[] = {10.9, 5.5, 2.77, 1.41, 1.17, 1.10, 1.04, 1.00, 0.975};  // 2^13 ... 2^21 lanes
  const double l = log2(lanes < 1 ? 1 : lanes);
  if (l <= 13) return f[0] * exp2(13 - l);  // below: the walk is one chain per lane, time goes with 1 / lanes
  if (l >= 21) return f[8];
  const int i = (int)l - 13;
  return f[i] + (f[i + 1] - f[i]) * (l - (13 + i));
}
// the group's inversion (fe_inv: about 16 400 VALU instructions, the same for every kernel) in keys' worth of the kernel's own per-key work.
// Every hashing type keeps the measured 5 (a 3 117-op key: 16 400 / 3 117 = 5.3).  A public key is the static per-key count of its kernel
// (tools/isa_mix.py --pub: the `which` loop + half the table loop's own body + half the prefix loop): 813 VALU instructions without the
// endomorphism, 692 + 3 x 196 (the image loop) + 253 = 1 533 per walked key with it - 16 400 / 813 = 20 and 16 400 / 1 533 = 11.
// These two are STATIC estimates (instruction counts of the assembly), standing in for the measured per-key count until a counter run
// (tools/bench_pub.py add 28 under SQ_INSTS_VALU) gives it.  Results never depend on it: it only picks the half group.
static double inv_keys_worth(u32 flags) {
  if (flags & ECL_PUB) return (flags & ECL_ENDO) ? 11.0 : 20.0;
  return 5.0;
}
static u32 auto_half_group(const ecl_hip* h, u64 nkeys) {
  u32 best = h->B;
  if (!h->B_auto) return best;
  double best_cost = 0;
  for (u32 B = h->B; B >= ECL_B_FLOOR; B >>= 1) {
    const u64 groups = (nkeys + 2ull * B - 1) / (2ull * B);
    const double lanes = groups < h->Tmax ? (double)groups : (double)h->Tmax;
    const double cost = lane_factor(lanes) * (1.0 + inv_keys_worth(h->flags) / (2.0 * B));
    if (B == h->B || cost < best_cost * 0.995) best = B, best_cost = cost;  // a smaller half group has to win by more than noise
    if (groups >= h->Tmax) break;  // every lane already has a group of its own: halving further only adds inversions
  }
  return best;
}
static void call_geometry(const ecl_hip* h, u64 nkeys, u32& B, u32& nb, u32& T) {
  B = auto_half_group(h, nkeys);
  const u64 group = 2ull * B, ngroups = (nkeys + group - 1) / group;
  // nb groups per lane, then the smallest lane count (multiple of 256) that covers the range: no lane idles
  // through a mostly masked last group
  nb = (u32)((ngroups + h->Tmax - 1) / h->Tmax);
  T = (u32)(((ngroups + nb - 1) / nb + 255) & ~255ull);
  if (T > h->Tmax) T = h->Tmax;
}
// what call_geometry can represent: the group count must not wrap and groups per lane must fit 32 bits
// (a caller-set geometry of 2 x 256 lanes reaches that at 2^42 keys; the default one never does below 2^63)
static bool nkeys_ok(const ecl_hip* h, u64 nkeys) {
  if (nkeys > (1ull << 63)) return false;
  const u32 B = auto_half_group(h, nkeys);
  const u64 ngroups = (nkeys + 2ull * B - 1) / (2ull * B);
  return (ngroups + h->Tmax - 1) / h->Tmax < (1ull << 32);
}
extern "C" int ecl_hip_plan_geometry(ecl_hip* h, uint64_t nkeys, uint32_t* half_group, uint32_t* lanes, uint32_t* groups_per_lane) {
  if (!h || nkeys == 0) return ECL_E_ARG;
  HIPCHK(h, hipSetDevice(h->dev));
  int rc = default_lanes(h);
  if (rc != ECL_OK) return rc;
  if (!nkeys_ok(h, nkeys)) return ECL_E_ARG;
  u32 B, nb, T;
  call_geometry(h, nkeys, B, nb, T);
  if (half_group) *half_group = B;
  if (lanes) *lanes = T;
  if (groups_per_lane) *groups_per_lane = nb;
  return ECL_OK;
}

// device buffers of a call with that geometry: lane centres and prefix-product chains
// the chains of the add walk and of the herd: `need` 16-byte elements and half as many words
static int ensure_scratch(ecl_hip* h, size_t need) {
  if (h->d_scr.n >= need && h->d_scr2.n >= need / 2) return ECL_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, h->d_scr.grow(need));
  HIPCHK(h, h->d_scr2.grow(need / 2));
  return ECL_OK;
}
static int ensure_walk_buffers(ecl_hip* h, u32 B, u32 T) {
  if (h->d_cxy.n < (size_t)T * 4) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->walk_valid = false;
    HIPCHK(h, h->d_cxy.grow((size_t)T * 4));
  }
  if (h->d_ctab.n < (size_t)T * 4) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->ctab_valid = false, h->aux_B = h->aux_T = 0;
    HIPCHK(h, h->d_ctab.grow((size_t)T * 4));
  }
  return ensure_scratch(h, (size_t)T * B * 2);
}

static int ensure_gtable(ecl_hip* h);
static int tr_reserve(ecl_hip* h, uint64_t nkeys);
static int tr_add_core(ecl_hip* h, const u256& k0, uint64_t nkeys, ecl_found* out, uint32_t cap, uint32_t* nout);

extern "C" int ecl_hip_reserve(ecl_hip* h, uint64_t nkeys, uint32_t cap) {
  if (!h || nkeys == 0 || cap > ECL_CAP_MAX) return ECL_E_ARG;
  HIPCHK(h, hipSetDevice(h->dev));
  int rc;
  if ((rc = default_lanes(h)) != ECL_OK) return rc;
  if ((rc = ensure_table(h)) != ECL_OK) return rc;
  if ((rc = ensure_gtable(h)) != ECL_OK) return rc;
  if (!nkeys_ok(h, nkeys)) return ECL_E_ARG;
  if ((rc = ensure_found(h, raw_cap_of(cap))) != ECL_OK) return rc;
  if (h->flags & ECL_TR) return tr_reserve(h, nkeys);
  u32 B, nb, T;
  call_geometry(h, nkeys, B, nb, T);
  return ensure_walk_buffers(h, B, T);
}

// one launch of the search kernel over exactly the keys k0, k0 + s, ..., k0 + (nkeys - 1) s  (k0 reduced mod n), in front of the
// collect() of the call frame `f`: geometry, buffers, the walk positioned at k0 (or continued), the kernel queued on h->stream, the walk
// state moved on.  slab: null, or where a Taproot call's emit kernel puts this launch's points, under the mark h->tr_epoch (tr_emit).
struct add_launched {
  int rc;
  bool continued;  // the resident walk was continued: no set-up
  add_launched(int rc_, bool continued_ = false) : rc(rc_), continued(continued_) {}
};
static add_launched add_launch(ecl_hip* h, const call_frame& f, const u256& k0, uint64_t nkeys, u32* slab) {
  int rc;
  if ((rc = default_lanes(h)) != ECL_OK) return rc;
  if (!nkeys_ok(h, nkeys)) {
    h->err = "nkeys too large for one call with this geometry";
    return ECL_E_ARG;
  }
  if ((rc = ensure_table(h)) != ECL_OK) return rc;

  u32 B, nb, T;
  call_geometry(h, nkeys, B, nb, T);
  const u64 group = 2ull * B;
  if ((rc = ensure_walk_buffers(h, B, T)) != ECL_OK) return rc;

  const u256 s = sc_pow2(h->offs);
  const u64 walked = (u64)nb * T * group;
  {
    // The walk cannot represent the point at infinity: refuse a scan that contains the scalar 0 (mod n), like the
    // reference's range check (main.c:687-690).  j0 = offset of that key = -k0 / 2^offs (mod n).
    u256 j0 = sc_neg(k0);
    for (u32 i = 0; i < h->offs; ++i) j0 = sc_half(j0);
    if (!(j0.w[1] | j0.w[2] | j0.w[3]) && j0.w[0] < walked && j0.w[0] < nkeys + group) {
      h->err = "the scan contains the private key 0 (mod n)";
      return ECL_E_RANGE;
    }
  }
  bool cont = h->walk_valid && h->walk_T == T && h->walk_B == B && u256_eq(h->walk_next, k0);
  const bool origin = h->flags & ECL_ORIGIN;
  if (origin && memcmp(h->walk_origin, h->origin_w, sizeof h->origin_w) != 0) cont = false;  // another origin: re-position
  h->pin_counter.p[CW_ORIGIN_INF] = 0;
  if (!cont) {
    if ((rc = ensure_gtable(h)) != ECL_OK) return rc;
    HIPCHK(h, hipEventRecord(h->ev_s0, h->stream));
    if (h->aux_B != B || h->aux_T != T) {
      // jump = (T*2B*s)*G and the ladder 2^j * (2B*s)*G depend on the geometry only: kept across calls
      h->aux_B = h->aux_T = 0;
      const u256 d = sc_mul_u64(s, group);
      std::vector<u32> ks(33 * 8);
      words_of(&ks[0], sc_mul_u64(d, T));
      u256 l = d;
      for (int j = 0; j < 32; ++j) {
        words_of(&ks[(size_t)(1 + j) * 8], l);
        l = sc_add(l, l);
      }
      HIPCHK(h, hipMemcpyAsync(h->d_auxk.p, ks.data(), ks.size() * sizeof(u32), hipMemcpyHostToDevice, h->stream));
      hipLaunchKernelGGL(k_mul_g, dim3(1), dim3(64), 0, h->stream, h->d_auxk.p, h->d_aux.p + 16, (u8*)nullptr, 33u);
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipMemcpyAsync(h->jump_host, h->d_aux.p + 16, 16 * sizeof(u32), hipMemcpyDeviceToHost, h->stream));
      // ... and so do the multiples (g + 1) * D, g < T (D = 2B * 2^offs * G = the first ladder point): the lane centres C_0 = D, D = D
      if (B >= 8)
        hipLaunchKernelGGL(k_init_centres_batched, dim3((T / INIT_R + 255) / 256), dim3(256), 0, h->stream, h->d_aux.p + 32, h->d_aux.p + 32,
                           h->d_ctab.p, T, (u32*)h->d_scr.p);
      else
        hipLaunchKernelGGL(k_init_centres, dim3(T / 256), dim3(256), 0, h->stream, h->d_aux.p + 32, h->d_aux.p + 32, h->d_ctab.p, T);
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipStreamSynchronize(h->stream));
      h->aux_B = B, h->aux_T = T, h->ctab_valid = true;
    }
    // C0 = (k0 + B*s)*G through the window table (19 additions, ~0.1 ms), the scalar travelling as a kernel argument;
    // then the lane centres C0 + g*D.  Nothing here waits for the host: the search kernel queues right behind.
    // (round 5) ... or, unless E = C0 - D is the point at infinity, E through the window table and the centres E + (g + 1) D from the cached
    // multiples of D: one affine addition per lane (k_init_centres_table)
    const u256 c0s = sc_add(k0, sc_mul_u64(s, B)), es = sc_add(c0s, sc_neg(sc_mul_u64(s, group)));
    const bool from_table = h->ctab_valid && (es.w[0] | es.w[1] | es.w[2] | es.w[3]) != 0;
    scalar_arg c0;
    words_of(c0.w, from_table ? es : c0s);
    hipLaunchKernelGGL(k_mul_window_one, dim3(1), dim3(64), 0, h->stream, c0, h->d_gtab.p, h->d_aux.p);
    HIPCHK(h, hipGetLastError());
    if (origin) {  // the base point shifted by O; the flag comes home with the call's one wait (add_core)
      origin_arg o;
      memcpy(o.w, h->origin_w, sizeof o.w);
      hipLaunchKernelGGL(k_origin_add, dim3(1), dim3(64), 0, h->stream, h->d_aux.p, o, h->d_aux.p + ECL_AUX_WORDS);
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipMemcpyAsync(h->pin_counter.p + CW_ORIGIN_INF, h->d_aux.p + ECL_AUX_WORDS, sizeof(u32), hipMemcpyDeviceToHost, h->stream));
      memcpy(h->walk_origin, h->origin_w, sizeof h->walk_origin);
    }
    if (from_table && T >= (1u << 19))
      hipLaunchKernelGGL(k_init_centres_table<8u>, dim3((T / 8u + 255) / 256), dim3(256), 0, h->stream, h->d_aux.p, h->d_ctab.p, h->d_cxy.p, T);
    else if (from_table)
      hipLaunchKernelGGL(k_init_centres_table<4u>, dim3((T / 4u + 255) / 256), dim3(256), 0, h->stream, h->d_aux.p, h->d_ctab.p, h->d_cxy.p, T);
    else if (B >= 8)  // the chain scratch (T * B * 36 bytes) holds the 144 bytes per lane the batched set-up parks
      hipLaunchKernelGGL(k_init_centres_batched, dim3((T / INIT_R + 255) / 256), dim3(256), 0, h->stream, h->d_aux.p, h->d_aux.p + 32,
                         h->d_cxy.p, T, (u32*)h->d_scr.p);
    else
      hipLaunchKernelGGL(k_init_centres, dim3(T / 256), dim3(256), 0, h->stream, h->d_aux.p, h->d_aux.p + 32, h->d_cxy.p, T);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev_s1, h->stream));
    h->walk_T = T, h->walk_B = B;
  }
  add_args a = f.args();
  a.tab = h->d_tab.p;
  memcpy(a.jump, h->jump_host, sizeof a.jump);
  a.cxy = h->d_cxy.p, a.scratch = h->d_scr.p, a.scratch2 = h->d_scr2.p;
  if (h->flags & ECL_PREFIX) a.prefix = prefix_of(h);
  if (h->flags & ECL_MASK) a.mask = mask_of(h);
  if (slab) a.slab = slab, a.epoch = h->tr_epoch;
  a.B = B, a.T = T, a.nb = nb, a.nkeys = nkeys;
  if (h->diag_drop) h->diag_drop = false, a.nb = nb - 1;  // (test hook: lane 0's last group is in the range, so keys go missing)
  if (!slab && (rc = f.reset()) != ECL_OK) return rc;  // a call of its own: its time starts behind the set-up (a Taproot call resets in front of its slabs)
  hipLaunchKernelGGL(pick_add_kernel(h->flags), dim3(T / ECL_ADD_BLOCK), dim3(ECL_ADD_BLOCK), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  // the centres now sit at the start of group nb*T + g: valid continuation only if the launch was exact
  h->walk_valid = walked == nkeys;
  if (h->walk_valid) h->walk_next = sc_add(k0, sc_mul_u64(s, walked));
  return add_launched(ECL_OK, cont);
}

static int add_core(ecl_hip* h, const u256& k0, uint64_t nkeys, ecl_found* out, uint32_t cap, uint32_t* nout) {
  *nout = 0;
  if (h->flags & ECL_TR) return tr_add_core(h, k0, nkeys, out, cap, nout);
  call_frame f = {h, "add_range", nullptr, nkeys, out, cap, nout, false, true};
  int rc;
  if ((rc = f.begin()) != ECL_OK) return rc;
  const add_launched l = add_launch(h, f, k0, nkeys, nullptr);
  if (l.rc != ECL_OK) return l.rc;
  if ((rc = f.collect()) != ECL_OK) return rc;
  rc = f.finish(1, l.continued ? 0 : 1);
  if (rc != ECL_E_COVERAGE && (h->flags & ECL_ORIGIN) && h->pin_counter.p[CW_ORIGIN_INF]) {  // origin + base point = the point at infinity: nothing was walked from it
    h->walk_valid = false;
    return f.refuse(ECL_E_RANGE, "the origin is the negative of the walk's base point");
  }
  return rc;
}

// ECL_ORIGIN: x and y of the origin (little-endian u64 limbs) checked on the host - both below p, y^2 = x^3 + 7 - and as canonical words
static bool origin_from_limbs(u32 w[16], const uint64_t xy[8]) {
  static const uint64_t P_LIMBS[4] = {0xfffffffefffffc2fULL, ~0ULL, ~0ULL, ~0ULL};
  for (int c = 0; c < 2; ++c) {
    if (u256_cmp(u256_from(xy + 4 * c), u256_from(P_LIMBS)) >= 0) return false;
    words_of(w + 8 * c, u256_from(xy + 4 * c));
  }
  const fe x = fe_from_words(w), y = fe_from_words(w + 8);
  fe seven = fe_zero();
  seven.n[0] = 7;
  fe rhs = fe_add(fe_mul(fe_sqr(x), x), seven);
  fe_normalize_weak(rhs);  // magnitude 1
  return fe_is_zero(fe_sub(fe_sqr(y), rhs));
}

#include "abi_herd.h"
#include "abi_lookahead.h"

// fingerprint of what a filter / a list holds, computed over ALL of its words where they are resident (k_fingerprint, aux_kernels.h: a 6 GB
// filter takes 2 ms): contexts share sweeps only if flags, stride, sizes and these agree.  A failure here only switches the look-ahead off.
static bool la_device_fingerprint(ecl_hip* h, const void* d_words, u64 nwords64, u64* fp) {
  devbuf<unsigned long long> acc;
  if (acc.grow(1) != hipSuccess ||hipMemsetAsync(acc.p, 0, 8, h->stream) != hipSuccess) return false;
  const u64 blocks = (nwords64 + 255) / 256;
  hipLaunchKernelGGL(k_fingerprint, dim3((unsigned)(blocks < 16384 ? (blocks ? blocks : 1) : 16384)), dim3(256), 0, h->stream, (const u64*)d_words, nwords64, acc.p);
  unsigned long long v = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&v, acc.p, 8, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess)
    return false;
  *fp = v;
  return true;
}
static void la_filter_changed(ecl_hip* h, const uint64_t*, uint64_t nwords) { h->la_key_valid = la_device_fingerprint(h, h->d_bloom.p, nwords, &h->la_bloom_fp); }
static void la_list_changed(ecl_hip* h, const uint32_t (*list)[5], uint64_t n) {
  h->la_list_fp = 0;
  if (!n) return;
  // the list's 20-byte entries as 64-bit words (n * 5 / 2, a last odd 32-bit word left to the entry count in the key: lists are sorted and
  // unique, so two lists that agree in everything but that word differ in it alone - it is added from the host copy)
  u64 fp = 0;
  if (!la_device_fingerprint(h, h->d_list.p, n * 5 / 2, &fp)) h->la_key_valid = false;
  if ((n * 5) & 1) fp += 0x9E3779B97F4A7C15ull * ((u64)list[n - 1][4] + 1);
  h->la_list_fp = fp;
}


extern "C" int ecl_hip_add_range(ecl_hip* h, const uint64_t start[4], uint64_t nkeys, ecl_found* out, uint32_t cap,
                                 uint32_t* nout) {
  if (!h || !start || (!out && cap) || !nout || cap > ECL_CAP_MAX) return ECL_E_ARG;
  *nout = 0;
  if (h->flags & ECL_HERD) {  // sixteen limbs, nkeys jumps, no filter (abi_herd.h)
    if (nkeys == 0) return ECL_OK;
    HIPCHK(h, hipSetDevice(h->dev));
    return count_call(h, nkeys, herd_add_core(h, start, nkeys, out, cap, nout));
  }
  if (!h->d_bloom.p) return ECL_E_NOBLOOM;
  if (nkeys == 0) return ECL_OK;
  HIPCHK(h, hipSetDevice(h->dev));
  const u256 k0 = sc_reduce(u256_from(start));
  if (h->flags & ECL_ORIGIN) {  // twelve limbs: the scalar, then x and y of the origin point
    u32 ow[16];
    if (!origin_from_limbs(ow, start + 4)) {  // (the context keeps the origin of the call before)
      h->err = "the origin is not a point of the curve";
      return ECL_E_ARG;
    }
    memcpy(h->origin_w, ow, sizeof ow);
  }
  // the walks of `bsgs`, prefix and mask contexts never take part in the look-ahead
  if (h->flags & (ECL_ORIGIN | ECL_INSERT | ECL_PREFIX | ECL_MASK)) return count_call(h, nkeys, add_core(h, k0, nkeys, out, cap, nout));
  return count_call(h, nkeys, la_dispatch(h, k0, nkeys, out, cap, nout));
}

#include "abi_mul.h"
#include "abi_seed.h"
#include "abi_gen.h"
#include "abi_tr.h"
#include "abi_diag.h"
