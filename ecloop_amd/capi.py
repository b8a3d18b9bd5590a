"""ctypes binding of the C ABI in include/ecloop_hip.h (libecloop_hip.so, built in-tree by ecloop_amd.build).

There is no CPU fallback: if the HIP library is missing or a call fails, this raises."""
import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ECLOOP_HIP_LIB") or os.path.join(PKG, "libecloop_hip.so")  # override: A/B builds

ADDR33, ADDR65, ENDO, P2SH, ETH, TR, PUB = 1, 2, 4, 16, 64, 128, 256
ORIGIN, INSERT = 512, 1024  # the two walks of `bsgs`, each valid only beside PUB alone (include/ecloop_hip.h)
HERD = 2048  # the herd of `kangaroo`, valid only beside PUB alone; ord_offs is then the number of distinguished-point bits
PREFIX = 4096  # the prefix filter in place of the bloom: beside ADDR33 / ADDR65 or ETH, with or without ENDO (include/ecloop_hip.h)
MASK = 8192  # the mask filter in place of the bloom: beside ETH alone, with or without ENDO / ORIGIN (include/ecloop_hip.h)
# the key derivation function of mul_batch_raw, a two-bit field (include/ecloop_hip.h): none = SHA-256; valid beside every context that has a `mul`
KDF_KECCAK, KDF_SHA3, KDF_CAMP2 = 0x4000, 0x8000, 0xC000
BIP39 = 0x10000  # the lines of mul_batch_raw are BIP39 phrases, lines[0] the derivation record (include/ecloop_hip.h: ECL_KDF_BIP39); not beside a KDF_* bit
GEN = 0x20000  # the lines of mul_batch_raw are generated on the device from a template (include/ecloop_hip.h: ECL_GEN); beside a KDF_* bit or none, not beside BIP39
KDF_FLAGS = {None: 0, "sha256": 0, "keccak": KDF_KECCAK, "sha3": KDF_SHA3, "camp2": KDF_CAMP2}
E_ARG = -1
E_NOBLOOM = -5
E_RANGE = -6
E_OVERFLOW = -4
E_COVERAGE = -8  # the device did not hash every key of the call (include/ecloop_hip.h, section 1)

U64x4 = C.c_uint64 * 4


class Found(C.Structure):
    _fields_ = [("key_offset", C.c_uint64), ("h160", C.c_uint32 * 5), ("endo", C.c_uint8),
                ("compressed", C.c_uint8), ("pad", C.c_uint8 * 2)]


FOUND_DTYPE = np.dtype([("key_offset", "<u8"), ("h160", "<u4", (5,)), ("endo", "u1"), ("compressed", "u1"),
                        ("pad", "u1", (2,))])
assert FOUND_DTYPE.itemsize == C.sizeof(Found) == 32

LABELS = {1: "addr33", 0: "addr65", 2: "p2sh", 3: "eth", 4: "p2tr", 5: "pub", 6: "dp"}  # ecl_found.compressed (the address type) -> label of the found line


def label_of(compressed):
    return LABELS[int(compressed)]

EXPORTS = [
    "ecl_hip_device_count", "ecl_hip_open", "ecl_hip_close", "ecl_hip_set_bloom", "ecl_hip_set_list", "ecl_hip_reserve", "ecl_hip_add_range",
    "ecl_hip_mul_batch", "ecl_hip_bloom_insert", "ecl_hip_get_bloom", "ecl_hip_set_geometry", "ecl_hip_get_geometry", "ecl_hip_get_timing", "ecl_hip_reset_timing", "ecl_hip_selftest", "ecl_hip_strerror",
    "ecl_hip_last_error", "ecl_hip_diag_fe", "ecl_hip_diag_mulg", "ecl_hip_diag_hash160", "ecl_hip_diag_bloom", "ecl_hip_diag_bloom_mod", "ecl_hip_set_lookahead", "ecl_hip_set_scan_end", "ecl_hip_get_lookahead_stats",
    "ecl_hip_get_setup_timing", "ecl_hip_get_mul_timing", "ecl_hip_bloom_insert_count", "ecl_hip_alloc_host", "ecl_hip_free_host", "ecl_hip_verify", "ecl_hip_sort_list", "ecl_hip_reserve_mul", "ecl_hip_mul_batch_raw", "ecl_hip_set_mul_window", "ecl_hip_get_mul_window", "ecl_hip_fetch_found", "ecl_hip_plan_geometry",
    "ecl_hip_p2sh_hash", "ecl_hip_get_coverage", "ecl_hip_diag_drop_round", "ecl_hip_verify_eth", "ecl_hip_verify_tr", "ecl_hip_diag_tr", "ecl_hip_diag_limbs",
]

_lib = None


class EclError(RuntimeError):
    """a failed library call; `code` is its return code (ECL_E_*: E_COVERAGE for a call whose keys were not all hashed), None when the
    failure is not a return code"""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EclError(f"{LIB_PATH} is missing: build it with `python -m ecloop_amd.build` "
                       "(there is no CPU fallback for the hot path)")
    lib = C.CDLL(LIB_PATH)
    P = C.c_void_p
    lib.ecl_hip_device_count.restype = C.c_int
    lib.ecl_hip_open.argtypes = [C.POINTER(P), C.c_int, C.c_uint32, C.c_uint32]
    lib.ecl_hip_close.argtypes = [P]
    lib.ecl_hip_close.restype = None
    lib.ecl_hip_set_bloom.argtypes = [P, C.c_void_p, C.c_uint64]
    lib.ecl_hip_set_list.argtypes = [P, C.c_void_p, C.c_uint64]
    lib.ecl_hip_reserve.argtypes = [P, C.c_uint64, C.c_uint32]
    lib.ecl_hip_add_range.argtypes = [P, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.ecl_hip_mul_batch.argtypes = [P, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.ecl_hip_fetch_found.argtypes = [P, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.ecl_hip_bloom_insert.argtypes = [P, C.c_void_p, C.c_uint64]
    lib.ecl_hip_get_bloom.argtypes = [P, C.c_void_p, C.c_uint64]
    lib.ecl_hip_bloom_insert_count.argtypes = [P, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.ecl_hip_set_geometry.argtypes = [P, C.c_uint32, C.c_uint32]
    lib.ecl_hip_get_geometry.argtypes = [P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.ecl_hip_plan_geometry.argtypes = [P, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.ecl_hip_get_timing.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.ecl_hip_reset_timing.argtypes = [P]
    lib.ecl_hip_get_setup_timing.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.ecl_hip_get_mul_timing.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.ecl_hip_get_coverage.argtypes = [P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.ecl_hip_diag_drop_round.argtypes = [P]
    lib.ecl_hip_set_lookahead.argtypes = [P, C.c_uint64]
    lib.ecl_hip_set_scan_end.argtypes = [P, C.c_void_p]
    lib.ecl_hip_get_lookahead_stats.argtypes = [P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.ecl_hip_set_mul_window.argtypes = [P, C.c_uint32]
    lib.ecl_hip_reserve_mul.argtypes = [P, C.c_uint32, C.c_uint32]
    lib.ecl_hip_sort_list.argtypes = [P, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.ecl_hip_mul_batch_raw.argtypes = [P, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.ecl_hip_get_mul_window.argtypes = [P, C.POINTER(C.c_uint32)]
    lib.ecl_hip_verify.argtypes = [P, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ecl_hip_p2sh_hash.argtypes = [P, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.ecl_hip_verify_eth.argtypes = [P, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.ecl_hip_verify_tr.argtypes = [P, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.ecl_hip_diag_tr.argtypes = [P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.ecl_hip_alloc_host.argtypes = [C.c_size_t]
    lib.ecl_hip_alloc_host.restype = C.c_void_p
    lib.ecl_hip_free_host.argtypes = [C.c_void_p]
    lib.ecl_hip_free_host.restype = None
    lib.ecl_hip_selftest.argtypes = [P]
    lib.ecl_hip_strerror.argtypes = [C.c_int]
    lib.ecl_hip_strerror.restype = C.c_char_p
    lib.ecl_hip_last_error.argtypes = [P]
    lib.ecl_hip_last_error.restype = C.c_char_p
    lib.ecl_hip_diag_fe.argtypes = [P, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.ecl_hip_diag_limbs.argtypes = [P, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.ecl_hip_diag_mulg.argtypes = [P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.ecl_hip_diag_hash160.argtypes = [P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.ecl_hip_diag_bloom.argtypes = [P, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.ecl_hip_diag_bloom_mod.argtypes = [P, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]
    _lib = lib
    return lib


def limbs(v):
    """python int -> 4 little-endian u64 limbs (the reference's `fe`)"""
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def limbs_array(vals):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def ints_of(arr):
    return [sum(int(r[i]) << (64 * i) for i in range(4)) for r in arr]


class Device:
    """One GPU context (ecl_hip handle)."""

    def __init__(self, device=0, a33=True, a65=False, endo=False, ord_offs=0, p2sh=False, eth=False, tr=False, pub=False, origin=False,
                 insert=False, herd=False, prefix=False, mask=False, kdf=None, bip39=False, gen=False):
        if kdf not in KDF_FLAGS:
            raise ValueError("kdf is None (SHA-256), 'keccak', 'sha3' or 'camp2'")
        if gen and (bip39 or origin or insert or herd or prefix or mask):
            raise ValueError("gen goes with the contexts that have a `mul`, with or without a kdf: not with bip39, origin, insert, herd, prefix or mask")
        self.gen = bool(gen)
        if bip39 and (KDF_FLAGS[kdf] or origin or insert or herd or prefix or mask):
            raise ValueError("bip39 goes with the contexts that have a `mul`, and not with a kdf: not with origin, insert, herd, prefix or mask")
        self.bip39 = bool(bip39)
        if KDF_FLAGS[kdf] and (origin or insert or herd or prefix or mask):
            raise ValueError("a kdf goes with the contexts that have a `mul`: not with origin, insert, herd, prefix or mask")
        self.kdf = kdf if KDF_FLAGS[kdf] else None
        if prefix and (p2sh or tr or pub or insert or herd or not (a33 or a65 or eth)):
            raise ValueError("the prefix filter goes with a33 / a65 or with eth: Device(prefix=True), Device(a33=False, eth=True, prefix=True)")
        if mask and (prefix or a33 or a65 or p2sh or tr or pub or insert or herd or not eth):
            raise ValueError("the mask filter goes with eth alone: Device(a33=False, eth=True, mask=True)")
        self.prefix, self.mask = bool(prefix), bool(mask)
        self.splitkey = bool((prefix or mask) and origin)  # the split-key search: the prefix / mask walk from an origin (twelve limbs per start and per verify entry)
        if pub and (a33 or a65 or p2sh or eth or tr):  # (before the library is asked)
            raise ValueError("public keys are searched alone: Device(a33=False, pub=True), with or without endo")
        if (origin or insert) and not self.splitkey and (not pub or endo or (origin and insert)):
            raise ValueError("origin and insert are the walks of bsgs: Device(a33=False, pub=True, origin=True) or (..., insert=True), no endo")
        if herd and (not pub or endo or origin or insert or not 0 <= ord_offs <= 32):
            raise ValueError("herd is the walk of kangaroo: Device(a33=False, pub=True, herd=True, ord_offs=dp), dp = 0 ... 32, no endo, origin or insert")
        self.origin, self.insert, self.herd = bool(origin), bool(insert), bool(herd)
        self.lib = load()
        self.h = C.c_void_p()
        self.a33, self.a65, self.endo, self.p2sh, self.eth, self.tr = bool(a33), bool(a65), bool(endo), bool(p2sh), bool(eth), bool(tr)
        self.pub = bool(pub)
        if eth and (a33 or a65 or p2sh):
            raise ValueError("eth is searched alone: Device(a33=False, eth=True)")
        if tr and (a33 or a65 or p2sh or eth or endo):
            raise ValueError("Taproot is searched alone and without the endomorphism: Device(a33=False, tr=True)")
        flags = (ADDR33 if a33 else 0) | (ADDR65 if a65 else 0) | (P2SH if p2sh else 0) | (ETH if eth else 0) | (TR if tr else 0) | (PUB if pub else 0) | (ENDO if endo else 0) | \
                (ORIGIN if origin else 0) | (INSERT if insert else 0) | (HERD if herd else 0) | (PREFIX if prefix else 0) | (MASK if mask else 0) | KDF_FLAGS[kdf] | (BIP39 if bip39 else 0) | (GEN if gen else 0)
        rc = self.lib.ecl_hip_open(C.byref(self.h), device, flags, ord_offs)
        if rc != 0:
            msg = self.lib.ecl_hip_last_error(self.h).decode() if self.h else ""
            if self.h:
                self.lib.ecl_hip_close(self.h)
                self.h = None
            raise EclError(f"ecl_hip_open(device={device}): {self.lib.ecl_hip_strerror(rc).decode()} {msg}", rc)

    def _chk(self, rc, allow=()):
        if rc != 0 and rc not in allow:
            raise EclError(f"{self.lib.ecl_hip_strerror(rc).decode()}: {self.lib.ecl_hip_last_error(self.h).decode()}", rc)
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.lib.ecl_hip_close(self.h)
            self.h = None

    __del__ = close

    def set_bloom(self, words):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        self._chk(self.lib.ecl_hip_set_bloom(self.h, w.ctypes.data, len(w)))

    def set_prefixes(self, ranges):
        """the range table of a Device(prefix=True): (n, 10) uint32, lo[5] then hi[5] per range, most significant word first, sorted by
        lo and disjoint (engine.prefix_ranges plans one from patterns)"""
        R = np.ascontiguousarray(ranges, dtype=np.uint32)
        if not self.prefix or R.ndim != 2 or R.shape[1] != 10:
            raise ValueError("set_prefixes takes an (n, 10) uint32 table on a Device(prefix=True)")
        self._chk(self.lib.ecl_hip_set_bloom(self.h, R.ctypes.data, 5 * len(R)))

    def set_masks(self, table):
        """the mask table of a Device(eth=True, mask=True): (n, 10) uint32, m[5] then v[5] per entry, most significant word first, 1 <= n <= 16,
        no bit of v outside m, no entry twice (engine.mask_table plans one from patterns)"""
        M = np.ascontiguousarray(table, dtype=np.uint32)
        if not self.mask or M.ndim != 2 or M.shape[1] != 10:
            raise ValueError("set_masks takes an (n, 10) uint32 table on a Device(eth=True, mask=True)")
        self._chk(self.lib.ecl_hip_set_bloom(self.h, M.ctypes.data, 5 * len(M)))

    def set_list(self, hashes):
        """sorted unique (n x 5) uint32 hash list for the on-device exact confirm; None / empty removes it"""
        H = np.zeros((0, 5), np.uint32) if hashes is None else np.ascontiguousarray(hashes, dtype=np.uint32).reshape(-1, 5)
        self._chk(self.lib.ecl_hip_set_list(self.h, H.ctypes.data if len(H) else None, len(H)))

    def reserve(self, nkeys, cap=4096):
        """allocate the device buffers of a later add_range(nkeys) now"""
        self._chk(self.lib.ecl_hip_reserve(self.h, nkeys, cap))

    def bloom_insert(self, hashes):
        H = np.ascontiguousarray(hashes, dtype=np.uint32).reshape(-1, 5)
        self._chk(self.lib.ecl_hip_bloom_insert(self.h, H.ctypes.data, len(H)))

    def bloom_insert_count(self, hashes):
        """blf-gen's insert loop (utils.c:455-470) on the device -> number of hashes that were new, in input order"""
        H = np.ascontiguousarray(hashes, dtype=np.uint32).reshape(-1, 5)
        added = C.c_uint64()
        self._chk(self.lib.ecl_hip_bloom_insert_count(self.h, H.ctypes.data, len(H), C.byref(added)))
        return added.value

    def get_bloom(self, nwords):
        w = np.zeros(nwords, dtype=np.uint64)
        self._chk(self.lib.ecl_hip_get_bloom(self.h, w.ctypes.data, nwords))
        return w

    def set_geometry(self, half_group=0, max_lanes=0):
        self._chk(self.lib.ecl_hip_set_geometry(self.h, half_group, max_lanes))

    def geometry(self):
        """-> (half_group, lanes); one sweep = lanes * 2 * half_group keys"""
        b, t = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.ecl_hip_get_geometry(self.h, C.byref(b), C.byref(t)))
        return b.value, t.value

    def plan_geometry(self, nkeys):
        """-> (half_group, lanes, groups per lane) that add_range would use for a call of nkeys keys"""
        b, t, nb = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.lib.ecl_hip_plan_geometry(self.h, nkeys, C.byref(b), C.byref(t), C.byref(nb)))
        return b.value, t.value, nb.value

    def add_range(self, start, nkeys, cap=4096, origin=None, herd=None):
        """-> (records as numpy structured array, total hit count). Raises on overflow unless total <= cap.
        A context opened with origin=True takes origin=(x, y), the affine origin point O: the call walks O + (start + j * stride) G.  One
        opened with insert=True sets the keys' filter bits and reports nothing (total 0).  One opened with herd=True takes start=None and herd=(B, Q, seed, herd_log2, jump_bits, spread_bits), Q = (x, y),
        and nkeys is the number of jumps, a multiple of 2^herd_log2 (include/ecloop_hip.h: ECL_HERD); the records are distinguished points."""
        out = np.zeros(cap, dtype=FOUND_DTYPE)
        n = C.c_uint32()
        if self.origin != (origin is not None):
            raise ValueError("add_range(origin=(x, y)) goes with Device(origin=True), and only with it")
        if self.herd != (herd is not None):
            raise ValueError("add_range(herd=(B, Q, seed, herd_log2, jb, sb)) goes with Device(herd=True), and only with it")
        if herd is not None:
            B, Q, seed, herd_log2, jb, sb = herd
            s = np.concatenate([limbs(B), limbs(Q[0]), limbs(Q[1]), np.array([seed & 0xFFFFFFFFFFFFFFFF, herd_log2, jb, sb], dtype=np.uint64)])
        else:
            s = limbs(start) if origin is None else np.concatenate([limbs(start), limbs(origin[0]), limbs(origin[1])])
        rc = self.lib.ecl_hip_add_range(self.h, s.ctypes.data, nkeys, out.ctypes.data, cap, C.byref(n))
        self._chk(rc, allow=(E_OVERFLOW,))
        return out[: min(n.value, cap)], n.value

    def set_lookahead(self, max_keys):
        """look-ahead over small contiguous jobs: sweeps of up to max_keys keys (0 = off, else 2^22 .. 2^32; default 2^30)"""
        self._chk(self.lib.ecl_hip_set_lookahead(self.h, max_keys))

    def set_scan_end(self, end):
        """hint: the scalar at which the scan stops handing out jobs (None withdraws it)"""
        e = limbs(end) if end is not None else None
        self._chk(self.lib.ecl_hip_set_scan_end(self.h, e.ctypes.data if e is not None else None))

    def lookahead_stats(self):
        """-> (sweeps run by this context, their keys, calls answered from a sweep, their keys)"""
        v = [C.c_uint64() for _ in range(4)]
        self._chk(self.lib.ecl_hip_get_lookahead_stats(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def fetch_found(self, first, n):
        """records [first, first + n) of the last add_range / mul_batch call that are still on the device (after an overflow:
        the call itself delivered [0, cap)); fewer come back only if the call produced more than the device kept"""
        out = np.zeros(n, dtype=FOUND_DTYPE)
        got = C.c_uint32()
        self._chk(self.lib.ecl_hip_fetch_found(self.h, first, out.ctypes.data, n, C.byref(got)))
        return out[: got.value]

    def mul_batch(self, scalars, cap=4096):
        k = limbs_array(scalars)
        out = np.zeros(cap, dtype=FOUND_DTYPE)
        n = C.c_uint32()
        rc = self.lib.ecl_hip_mul_batch(self.h, k.ctypes.data, len(k), out.ctypes.data, cap, C.byref(n))
        self._chk(rc, allow=(E_OVERFLOW,))
        return out[: min(n.value, cap)], n.value

    def mul_batch_raw(self, lines, cap=4096):
        """`mul -raw`: lines = list of bytes objects; their digests are the scalars (hashed on the device) - SHA-256, or on a
        Device(kdf="keccak" | "sha3" | "camp2") Keccak-256, SHA3-256 or Keccak-256 applied 2031 times (engine.kdf_digest is the definition)"""
        text = b"".join(lines)
        table = np.zeros(len(lines), dtype=np.uint64)
        at = 0
        for i, l in enumerate(lines):
            table[i] = at | (len(l) << 32)
            at += len(l)
        buf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        out = np.zeros(cap, dtype=FOUND_DTYPE)
        n = C.c_uint32()
        rc = self.lib.ecl_hip_mul_batch_raw(self.h, buf.ctypes.data, len(text), table.ctypes.data, len(lines), out.ctypes.data, cap, C.byref(n))
        self._chk(rc, allow=(E_OVERFLOW,))
        return out[: min(n.value, cap)], n.value

    @staticmethod
    def seed_record(path, passphrase=b"", reuse=False):
        """the derivation record of a Device(bip39=True) call (include/ecloop_hip.h: ECL_KDF_BIP39): magic, reuse, depth, pass_len, zero;
        the path's elements as little-endian u32; the passphrase"""
        return b"B39\0" + bytes([1 if reuse else 0, len(path), len(passphrase), 0]) + b"".join(int(e).to_bytes(4, "little") for e in path) + bytes(passphrase)

    def seed_batch(self, phrases, path, passphrase=b"", reuse=False, cap=4096):
        """phrases (bytes objects) -> (records, total) for the keys at `path` (a list of 32-bit elements, bit 31 = hardened): lines[0] is the
        record, key_offset of a record the index into `phrases`.  reuse=True: the phrases are those of the call before, only the path is
        walked again from the kept master nodes"""
        if not self.bip39:
            raise ValueError("seed_batch goes with Device(bip39=True)")
        if len(path) > 255 or len(passphrase) > 255:
            raise ValueError("a path of more than 255 elements or a passphrase of more than 255 bytes does not fit the record")
        return self.mul_batch_raw([self.seed_record(path, passphrase, reuse)] + list(phrases), cap=cap)

    def brain_batch(self, template, first, n, cap=4096):
        """the candidates first ... first + n - 1 of a template, generated and hashed on the device -> (records, total); key_offset of a
        record is its index - first.  template: positions (a list of lists of bytes objects: engine.parse_mask makes one from a mask) or
        the packed blob of engine.brain_table (include/ecloop_hip.h: ECL_GEN)"""
        if not self.gen:
            raise ValueError("brain_batch goes with Device(gen=True)")
        if not isinstance(template, (bytes, bytearray)):
            from .engine import brain_table
            template = brain_table(template)
        buf = np.frombuffer(bytes(template), dtype=np.uint8) if template else np.zeros(1, dtype=np.uint8)
        start = np.array([first], dtype=np.uint64)
        out = np.zeros(cap, dtype=FOUND_DTYPE)
        got = C.c_uint32()
        rc = self.lib.ecl_hip_mul_batch_raw(self.h, buf.ctypes.data, len(template), start.ctypes.data, n, out.ctypes.data, cap, C.byref(got))
        self._chk(rc, allow=(E_OVERFLOW,))
        return out[: min(got.value, cap)], got.value

    def set_mul_window(self, bits):
        """window width of this context's `mul` table (8..29 bits; 0 = automatic: 22, then 26 after 2^30 scalars)"""
        self._chk(self.lib.ecl_hip_set_mul_window(self.h, bits))

    def sort_list(self, h160):
        """(n, 5) uint32 hash160 words -> the sorted (compare_160 order), duplicate-free entries"""
        a = np.ascontiguousarray(h160, dtype=np.uint32).copy()
        kept = C.c_uint64()
        self._chk(self.lib.ecl_hip_sort_list(self.h, a.ctypes.data, len(a), C.byref(kept)))
        return a[: kept.value]

    def reserve_mul(self, n, cap=4096):
        self._chk(self.lib.ecl_hip_reserve_mul(self.h, n, cap))

    def mul_window(self):
        bits = C.c_uint32()
        self._chk(self.lib.ecl_hip_get_mul_window(self.h, C.byref(bits)))
        return bits.value

    def _verify_entries(self, ks, origin):
        """four limbs per scalar - or, on a Device(prefix=True, origin=True), twelve: the scalar, then x and y of its origin (one point (x, y)
        for all, or one per scalar; None in a list stands for the point at infinity)"""
        K = limbs_array(ks)
        if self.splitkey != (origin is not None):
            raise ValueError("verify(origin=...) goes with Device(prefix=True, origin=True) or Device(mask=True, origin=True), and only with them")
        if origin is None:
            return K
        pts = list(origin) if isinstance(origin, list) else [origin] * len(K)
        if len(pts) != len(K):
            raise ValueError("verify(origin=[...]): one origin per key")
        O = np.array([[0] * 8 if p is None else list(limbs(p[0])) + list(limbs(p[1])) for p in pts], dtype=np.uint64).reshape(-1, 8)
        return np.ascontiguousarray(np.concatenate([K, O], axis=1))

    def verify(self, ks, origin=None):
        """pk_verify_hash for a batch: -> (h33, h65, ok) of the scalars' public keys (window-table path); with origin= (a split-key
        device): of the points O + k G"""
        K = self._verify_entries(ks, origin)
        h33 = np.zeros((len(K), 5), dtype=np.uint32)
        h65 = np.zeros((len(K), 5), dtype=np.uint32)
        ok = np.zeros(len(K), dtype=np.uint8)
        self._chk(self.lib.ecl_hip_verify(self.h, K.ctypes.data, len(K), h33.ctypes.data, h65.ctypes.data, ok.ctypes.data))
        return h33, h65, ok

    def p2sh_hash(self, h33):
        """(n, 5) addr33 hash160 words -> (n, 5) P2SH-P2WPKH hashes hash160(0x00 0x14 || h33), computed on the device"""
        H = np.ascontiguousarray(h33, dtype=np.uint32).reshape(-1, 5)
        out = np.zeros_like(H)
        self._chk(self.lib.ecl_hip_p2sh_hash(self.h, H.ctypes.data, out.ctypes.data, len(H)))
        return out

    def verify_eth(self, ks, origin=None):
        """-> (addr, ok): the Ethereum address of each scalar's public key by verify's path (window-table sum, not the walk kernel); with
        origin= (a split-key device): of the points O + k G"""
        K = self._verify_entries(ks, origin)
        addr = np.zeros((len(K), 5), dtype=np.uint32)
        ok = np.zeros(len(K), dtype=np.uint8)
        self._chk(self.lib.ecl_hip_verify_eth(self.h, K.ctypes.data, len(K), addr.ctypes.data, ok.ctypes.data))
        return addr, ok

    def verify_tr(self, ks):
        """-> (qx, ok): the Taproot output key (n x 8 big-endian uint32 words) of each private key by verify's path, ok = 0 for k = 0 (mod n)
        or a tweak >= n"""
        K = limbs_array(ks)
        qx = np.zeros((len(K), 8), dtype=np.uint32)
        ok = np.zeros(len(K), dtype=np.uint8)
        self._chk(self.lib.ecl_hip_verify_tr(self.h, K.ctypes.data, len(K), qx.ctypes.data, ok.ctypes.data))
        return qx, ok

    def verify_pub(self, ks):
        """-> (x, parity, ok): the public key of each private key by the double-and-add kernel (diag_mulg: neither the walk nor the window
        sum) - x as n x 8 big-endian uint32 words (the first five are what a pub record's h160 holds), the parity of y, ok = 0 for k = 0 (mod n)"""
        xs, ys, ok = self.diag_mulg(ks)
        x = np.array([[(v >> (32 * (7 - j))) & 0xFFFFFFFF for j in range(8)] for v in xs], dtype=np.uint32).reshape(len(xs), 8)
        par = np.array([v & 1 for v in ys], dtype=np.uint8)
        return x, par, ok

    def diag_tr(self, xs, ys):
        """the two stages of the Taproot search path for affine points -> (tweaks as ints, output keys n x 8 big-endian words, ok)"""
        X, Y = limbs_array(xs), limbs_array(ys)
        T = np.zeros_like(X)
        qx = np.zeros((len(X), 8), dtype=np.uint32)
        ok = np.zeros(len(X), dtype=np.uint8)
        self._chk(self.lib.ecl_hip_diag_tr(self.h, X.ctypes.data, Y.ctypes.data, T.ctypes.data, qx.ctypes.data, ok.ctypes.data, len(X)))
        return ints_of(T), qx, ok

    def selftest(self):
        self._chk(self.lib.ecl_hip_selftest(self.h))

    def timing(self):
        ms, launches, keys = C.c_double(), C.c_uint64(), C.c_uint64()
        self._chk(self.lib.ecl_hip_get_timing(self.h, C.byref(ms), C.byref(launches), C.byref(keys)))
        return ms.value, launches.value, keys.value

    def coverage(self):
        """-> (requested, covered, device): keys / scalars of the calls since open, those whose device count was checked whole, and the
        keys this context's kernels counted (look-ahead sweeps whole); requested == covered on a sound device"""
        v = [C.c_uint64() for _ in range(3)]
        self._chk(self.lib.ecl_hip_get_coverage(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def diag_drop_round(self):
        """test hook: the next search launch runs one round short, so that the call fails with EclError(code=E_COVERAGE)"""
        self._chk(self.lib.ecl_hip_diag_drop_round(self.h))

    def reset_timing(self):
        self._chk(self.lib.ecl_hip_reset_timing(self.h))

    def setup_timing(self):
        """-> (ms spent in the set-up kernels of non-contiguous add_range calls, number of such calls)"""
        ms, n = C.c_double(), C.c_uint64()
        self._chk(self.lib.ecl_hip_get_setup_timing(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def mul_timing(self):
        """-> (ms of mul_batch on the device incl. the overlapped scalar copies, calls, scalars)"""
        ms, calls, n = C.c_double(), C.c_uint64(), C.c_uint64()
        self._chk(self.lib.ecl_hip_get_mul_timing(self.h, C.byref(ms), C.byref(calls), C.byref(n)))
        return ms.value, calls.value, n.value

    # ---- diagnostics
    def diag_fe(self, op, a, b=None):
        A = limbs_array(a)
        Bv = limbs_array(b) if b is not None else A
        R = np.zeros_like(A)
        self._chk(self.lib.ecl_hip_diag_fe(self.h, op, A.ctypes.data, Bv.ctypes.data, R.ctypes.data, len(A)))
        return ints_of(R)

    def diag_limbs(self, op, cases):
        """one operation of csrc/limb_ops.h on raw 9x29 limbs: cases = (n, 6, 9) uint32 -> (results (n, 4, 9) uint32, flags (n,) uint32);
        nothing is normalised on the way in or out"""
        X = np.ascontiguousarray(cases, dtype=np.uint32)
        if X.ndim != 3 or X.shape[1:] != (6, 9):
            raise ValueError("cases must have the shape (n, 6, 9)")
        out = np.zeros((len(X), 4, 9), dtype=np.uint32)
        flag = np.zeros(len(X), dtype=np.uint32)
        self._chk(self.lib.ecl_hip_diag_limbs(self.h, op, X.ctypes.data, out.ctypes.data, flag.ctypes.data, len(X)))
        return out, flag

    def diag_mulg(self, ks):
        K = limbs_array(ks)
        X, Y = np.zeros_like(K), np.zeros_like(K)
        ok = np.zeros(len(K), dtype=np.uint8)
        self._chk(self.lib.ecl_hip_diag_mulg(self.h, K.ctypes.data, X.ctypes.data, Y.ctypes.data, ok.ctypes.data, len(K)))
        return ints_of(X), ints_of(Y), ok

    def diag_hash160(self, xs, ys):
        X, Y = limbs_array(xs), limbs_array(ys)
        h33 = np.zeros((len(X), 5), dtype=np.uint32)
        h65 = np.zeros((len(X), 5), dtype=np.uint32)
        self._chk(self.lib.ecl_hip_diag_hash160(self.h, X.ctypes.data, Y.ctypes.data, h33.ctypes.data, h65.ctypes.data, len(X)))
        return h33, h65

    def diag_bloom(self, hashes):
        H = np.ascontiguousarray(hashes, dtype=np.uint32).reshape(-1, 5)
        hit = np.zeros(len(H), dtype=np.uint8)
        self._chk(self.lib.ecl_hip_diag_bloom(self.h, H.ctypes.data, hit.ctypes.data, len(H)))
        return hit

    def diag_bloom_mod(self, nwords, xs):
        X = np.ascontiguousarray(xs, dtype=np.uint64)
        R = np.zeros_like(X)
        self._chk(self.lib.ecl_hip_diag_bloom_mod(self.h, nwords, X.ctypes.data, R.ctypes.data, len(X)))
        return R
