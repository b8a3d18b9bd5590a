"""Host-side mirror of the reference's command drivers (vladkens/ecloop main.c), driving the GPU through the C ABI.

What lives here is what the reference keeps on the host: filter loading, job arithmetic, the
sorted-list confirm, calc_priv, the pk_verify_hash self-check, the found sink, range sharding across GPUs.
All curve / hash work goes to the device (ecloop_amd.capi.Device); nothing here can compute a hash160 on the CPU.
Names follow the reference: load_filter, cmd_add, cmd_mul, calc_priv, pk_verify_hash, ctx_write_found.
"""
import hashlib
import hmac
import math
import os
import struct

import numpy as np

from .capi import Device, EclError, label_of

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
P = 2**256 - 2**32 - 977
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72  # A1, lib/ecc.c:36 (A2 = A1^2 mod n)
GROUP_INV_SIZE = 2048  # main.c:17
MAX_JOB_SIZE = 2 * 1024 * 1024  # main.c:16
BLF_MAGIC, BLF_VERSION = 0x45434246, 1  # lib/utils.c:274-275

# ----------------------------------------------------------------------------------------------- bloom filter (host side)


def blf_size_words(n):
    """lib/utils.c:421-427: m = n*ln(1e-9)/ln(1/2^ln2) bits, ceil to 64-bit words"""
    p = 1.0 / float(1000000000)
    m = int(n * math.log(p) / math.log(1.0 / math.pow(2.0, math.log(2.0))))
    return (m + 63) // 64


def blf_indices(h160):
    """lib/utils.c:290-306: the 20 probe positions of each hash (N x 5 uint32 words) -> N x 20 uint64"""
    h = np.ascontiguousarray(h160, dtype=np.uint32).reshape(-1, 5).astype(np.uint64)
    a = [h[:, 0] << np.uint64(32) | h[:, 1], h[:, 2] << np.uint64(32) | h[:, 3], h[:, 4] << np.uint64(32) | h[:, 0],
         h[:, 1] << np.uint64(32) | h[:, 2], h[:, 3] << np.uint64(32) | h[:, 4]]
    cols = []
    for s in (24, 28, 36, 40):
        for j in range(5):
            cols.append((a[j] << np.uint64(s)) | (a[(j + 1) % 5] >> np.uint64(s)))
    return np.stack(cols, axis=1)


def blf_add_host(words, h160):
    """blf_add for small lists on the host (bit-identical to the device bulk insert)"""
    idx = blf_indices(h160).reshape(-1)
    size = np.uint64(len(words))
    np.bitwise_or.at(words, ((idx >> np.uint64(6)) % size).astype(np.int64), np.uint64(1) << (idx & np.uint64(63)))


def blf_save(path, words):
    """lib/utils.c:328-360"""
    words = np.ascontiguousarray(words, dtype="<u8")
    with open(path, "wb") as f:
        f.write(struct.pack("<IIQ", BLF_MAGIC, BLF_VERSION, len(words)))
        f.write(words.tobytes())


def blf_load(path):
    """lib/utils.c:362-396"""
    with open(path, "rb") as f:
        head = f.read(16)
        if len(head) != 16:
            raise ValueError("failed to read bloom filter header")
        magic, ver, size = struct.unpack("<IIQ", head)
        if magic != BLF_MAGIC or ver != BLF_VERSION:
            raise ValueError("invalid bloom filter version; create a new filter with blf-gen command")
        words = np.fromfile(f, dtype="<u8", count=size)
    if len(words) != size:
        raise ValueError("failed to read bloom filter bits")
    return words.astype(np.uint64)


class Filter:
    """ctx->blf + ctx->to_find_hashes (main.c:48-51). `hashes` is None in bloom-only mode."""

    def __init__(self, words, hashes=None):
        self.words = np.ascontiguousarray(words, dtype=np.uint64)
        self.hashes = hashes  # sorted unique (count x 5) uint32, or None
        # big-endian bytes of the 5 words compare like compare_160 (lib/addr.c:18-26): binary search on 20-byte keys
        self._keys = None if hashes is None else np.ascontiguousarray(np.asarray(hashes, dtype=">u4")).view("S20").reshape(-1)

    @property
    def count(self):
        return 0 if self.hashes is None else len(self.hashes)

    def confirm(self, h160):
        """second stage of ctx_check_hash (main.c:212-216): exact membership in list mode, always true in bloom mode"""
        if self._keys is None:
            return True
        key = np.asarray([int(v) for v in h160], dtype=">u4").tobytes()
        i = int(np.searchsorted(self._keys, np.bytes_(key)))
        return i < len(self._keys) and self._keys[i].ljust(20, b"\0") == key


def parse_hash_list(path):
    """main.c:96-110. fgets into a 41-byte buffer consumes a long line in 40-character chunks and every full chunk
    becomes an entry; short chunks are skipped.  Chunks that are not clean hex (the reference sscanf's garbage out of
    them: a quirk, it inflates the banner count by one for data/btc-bw-hash) are dropped here."""
    out = []
    with open(path, "rb") as f:
        for raw in f.read().decode("latin1").split("\n"):
            for i in range(0, max(len(raw), 1), 40):
                ch = raw[i : i + 40]
                if len(ch) != 40:
                    continue
                try:
                    out.append([int(ch[j : j + 8], 16) for j in range(0, 40, 8)])
                except ValueError:
                    pass
    return out


def load_filter(path):
    """main.c:71-131: `.blf` -> bloom-only mode; anything else -> hex list, sorted + deduplicated, plus an in-memory
    bloom of 2*count words."""
    if not path:
        raise ValueError("missing filter file")
    if not os.path.exists(path):
        raise ValueError(f"failed to open filter file: {path}")
    if os.path.splitext(path)[1] == ".blf":
        return Filter(blf_load(path))
    hs = np.array(parse_hash_list(path), dtype=np.uint32).reshape(-1, 5)
    if len(hs) == 0:
        raise ValueError("empty hash list")
    hs = np.unique(hs, axis=0)  # lexicographic on the 5 words == compare_160 (lib/addr.c:18-26)
    words = np.zeros(len(hs) * 2, dtype=np.uint64)
    blf_add_host(words, hs)
    return Filter(words, hs)


# ----------------------------------------------------------------------------------------------- scalar helpers (host)


def calc_priv(start, stride, off, endo):
    """main.c:267-276 with python integers (the reference's non-reducing fe_modn_add is a representation quirk:
    the value is the same residue mod n)"""
    k = (start + off * stride) % N
    if endo in (2, 3):
        k = k * LAMBDA % N
    elif endo in (4, 5):
        k = k * LAMBDA % N * LAMBDA % N
    if endo in (1, 3, 5):
        k = (-k) % N
    return k


def parse_range(raw):
    """arg_search_range (main.c:666-701): hex `A:B`, A > 0x800, B <= p, A < B; default 0x800:p"""
    if raw is None:
        return GROUP_INV_SIZE, P
    if ":" not in raw:
        raise ValueError("invalid search range, use format: -r 8000:ffff")
    a, b = raw.split(":", 1)
    rs, re_ = scalar_from_hex(a), scalar_from_hex(b)
    if rs <= GROUP_INV_SIZE:
        raise ValueError("invalid search range, start <= 0x800")
    if re_ > P:
        raise ValueError("invalid search range, end > FE_P")
    if rs >= re_:
        raise ValueError("invalid search range, start >= end")
    return rs, re_


def scalar_from_hex(s):
    """fe_modn_from_hex (lib/ecc.c:81-95,262-265): right-to-left, non-hex characters skipped, at most 64 digits"""
    digits = [c for c in s if c in "0123456789abcdefABCDEF"][-64:]
    v = int("".join(digits), 16) if digits else 0
    return v - N if v >= N else v


def job_plan(range_s, range_e, stride=1):
    """cmd_add + cmd_add_worker (main.c:405-454): job_size = min(B-A, 2^21) (scalar units, whatever the stride);
    a job advances range_s by job_size*stride and jobs are handed out until range_s >= range_e; each job hashes
    ceil(job_size/2048)*2048 keys.  Returns (job_size, njobs, keys_hashed): the keys actually hashed are the
    contiguous run range_s + i*stride, i < keys_hashed."""
    span = range_e - range_s
    job = span if span < MAX_JOB_SIZE else MAX_JOB_SIZE
    njobs = (span + job * stride - 1) // (job * stride)
    per_job = (job + GROUP_INV_SIZE - 1) // GROUP_INV_SIZE * GROUP_INV_SIZE
    hashed = (njobs - 1) * job + per_job
    return job, njobs, hashed


def shard(total, rank, world, align=GROUP_INV_SIZE):
    """contiguous range partition of `total` keys over `world` GPUs: (offset, count) for `rank`"""
    per = (total + world - 1) // world
    per = (per + align - 1) // align * align
    lo = min(total, rank * per)
    hi = min(total, lo + per)
    return lo, hi - lo


def gather_found(lines, dist=None):
    """found lists of all ranks -> every rank (the reference's single found sink, main.c:182-203); host objects only"""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return list(lines)
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, list(lines))
    return [l for part in parts for l in part]


def max_over_ranks(seconds, dist=None):
    """wall time of the slowest rank (the job is done when the last shard is)"""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return float(seconds)
    import torch
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    t = torch.tensor([float(seconds)], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


# ----------------------------------------------------------------------------------------------- command drivers


# ----------------------------------------------------------------------------------------------- key derivation (mul -raw -kdf)
# The definition of the four functions, in plain Python (FIPS 202: the sponge with rate 136 and capacity 512 over Keccak-f[1600]): the key of
# a line is its digest read as a big-endian number.  sha256: the Bitcoin brain-wallet convention (the reference's -raw); keccak: Keccak-256,
# first pad byte 0x01 (old ethaddress, early ethercamp); sha3: SHA3-256, first pad byte 0x06; camp2: Keccak-256 applied 2031 times, each
# time to the 32 bytes of the digest before (the later ethercamp wallet).
KDF_NAMES = ("sha256", "keccak", "sha3", "camp2")
KDF_CAMP2_HASHES = 2031
_M64 = (1 << 64) - 1
_KECCAK_ROT = ((0, 36, 3, 41, 18), (1, 44, 10, 45, 2), (62, 6, 43, 15, 61), (28, 55, 25, 21, 56), (27, 20, 39, 8, 14))  # [x][y], FIPS 202 table 2
_KECCAK_RC = (0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
              0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
              0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
              0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008)


def _keccak_f(a):
    """a[x][y], permuted in place"""
    rol = lambda v, n: ((v << n) | (v >> (64 - n))) & _M64 if n else v
    for rc in _KECCAK_RC:
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        for x in range(5):
            d = c[(x - 1) % 5] ^ rol(c[(x + 1) % 5], 1)
            for y in range(5):
                a[x][y] ^= d
        b = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = rol(a[x][y], _KECCAK_ROT[x][y])
        for x in range(5):
            for y in range(5):
                a[x][y] = b[x][y] ^ (~b[(x + 1) % 5][y] & b[(x + 2) % 5][y])
        a[0][0] ^= rc


def _sponge256(msg, pad):
    a = [[0] * 5 for _ in range(5)]
    tail = bytearray(msg[len(msg) - len(msg) % 136:]) + bytes(136 - len(msg) % 136)
    tail[len(msg) % 136] ^= pad
    tail[135] ^= 0x80
    data = bytes(msg[: len(msg) - len(msg) % 136]) + bytes(tail)
    for at in range(0, len(data), 136):
        for i in range(17):
            a[i % 5][i // 5] ^= int.from_bytes(data[at + 8 * i: at + 8 * i + 8], "little")
        _keccak_f(a)
    return b"".join(a[i][0].to_bytes(8, "little") for i in range(4))


def kdf_digest(name, line):
    """the 32-byte digest that `mul -raw -kdf name` takes as the key of `line` (bytes)"""
    if name == "sha256":
        return hashlib.sha256(line).digest()
    if name == "keccak":
        return _sponge256(line, 0x01)
    if name == "sha3":
        return _sponge256(line, 0x06)
    if name == "camp2":
        d = _sponge256(line, 0x01)
        for _ in range(KDF_CAMP2_HASHES - 1):
            d = _sponge256(d, 0x01)
        return d
    raise ValueError("kdf is one of sha256, keccak, sha3, camp2")


# ----------------------------------------------------------------------------------------------- BIP39 phrases (seed)
# The definition of what a Device(bip39=True) derives, in plain Python: BIP39's seed of the phrase bytes as given (no NFKD, no word list, no
# checksum test), BIP32's master node and CKDpriv down the path.  A node BIP32 calls invalid gives the key 0.
BIP32_HARDENED = 1 << 31
BIP32_DEPTH_MAX = 10
BIP39_PASS_MAX = 99
SEED_COUNT_MAX = 1024
SEED_BATCH = 1 << 20
_G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)


def parse_path(text):
    """m/44'/0'/0'/0/0 (' or h: hardened) -> the list of 32-bit path elements, bit 31 = hardened; at most 10 of them"""
    parts = text.split("/")
    if parts[0] != "m" or len(parts) - 1 > BIP32_DEPTH_MAX:
        raise ValueError("a path is m, or m/ followed by at most 10 elements: %r" % text)
    out = []
    for p in parts[1:]:
        hard = p[-1:] in ("'", "h")
        digits = p[:-1] if hard else p
        if not digits.isdigit() or not digits.isascii() or int(digits) >= BIP32_HARDENED:
            raise ValueError("a path element is a number below 2^31, with ' or h for hardened: %r" % text)
        out.append(int(digits) | (BIP32_HARDENED if hard else 0))
    return out


def format_path(path):
    return "/".join(["m"] + ["%d'" % (e & (BIP32_HARDENED - 1)) if e & BIP32_HARDENED else "%d" % e for e in path])


def _pt_add(a, b):
    if a is None or b is None:
        return a if b is None else b
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def _ser_pub(k):
    acc, q = None, _G
    while k:
        if k & 1:
            acc = _pt_add(acc, q)
        q = _pt_add(q, q)
        k >>= 1
    return bytes([2 | (acc[1] & 1)]) + acc[0].to_bytes(32, "big")


def bip39_key(phrase, path, passphrase=b""):
    """the private key (int) a Device(bip39=True) derives for the phrase (bytes) at `path` (a list of elements, or text for parse_path);
    0 for a node BIP32 calls invalid"""
    if isinstance(path, str):
        path = parse_path(path)
    seed = hashlib.pbkdf2_hmac("sha512", bytes(phrase), b"mnemonic" + bytes(passphrase), 2048, 64)
    I = hmac.new(b"Bitcoin seed", seed, hashlib.sha512).digest()
    k, c = int.from_bytes(I[:32], "big"), I[32:]
    if not 0 < k < N:
        return 0
    for e in path:
        data = (b"\0" + k.to_bytes(32, "big") if e & BIP32_HARDENED else _ser_pub(k)) + e.to_bytes(4, "big")
        I = hmac.new(c, data, hashlib.sha512).digest()
        il = int.from_bytes(I[:32], "big")
        if il >= N or (il + k) % N == 0:
            return 0
        k, c = (il + k) % N, I[32:]
    return k


# ----------------------------------------------------------------------------------------------- generated pass phrases (brain)
# The mirror of ecloop_amd/host/gen_plan.h (the template is defined there).  A template is `positions`: a list of positions, each a list
# of alternatives (bytes objects).  Candidate i takes alternative d_p of position p, i = sum d_p * prod_{q > p} c_q: the last position
# runs fastest.
GEN_POS_MAX, GEN_ALT_LEN_MAX, GEN_L_MAX, GEN_NALT_MAX, GEN_POOL_MAX = 16, 255, 256, 1 << 22, 1 << 28
BRAIN_CALL = 1 << 24
_GEN_SPECIALS = b" !\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"
_GEN_LOWER, _GEN_UPPER, _GEN_DIGITS = bytes(range(97, 123)), bytes(range(65, 91)), b"0123456789"
GEN_CLASSES = {"l": _GEN_LOWER, "u": _GEN_UPPER, "d": _GEN_DIGITS, "h": b"0123456789abcdef", "s": _GEN_SPECIALS,
               "a": _GEN_LOWER + _GEN_UPPER + _GEN_DIGITS + _GEN_SPECIALS}


def brain_words(text):
    """the words of a word list (bytes): cut at newlines as `mul -raw` cuts lines - one '\\r' before the newline dropped, empty lines
    skipped, duplicates kept"""
    words = [w[:-1] if w.endswith(b"\r") else w for w in bytes(text).split(b"\n")]
    words = [w for w in words if w]
    if any(len(w) > GEN_ALT_LEN_MAX for w in words):
        raise ValueError("a word is longer than 255 bytes")
    return words


def _brain_set(spec, name):
    """-1 ... -4: @file (its words), or literal bytes and classes -> one-byte alternatives in the order given, none twice"""
    spec = spec.encode("latin-1") if isinstance(spec, str) else bytes(spec)
    if spec[:1] == b"@":
        words = brain_words(open(spec[1:].decode("latin-1"), "rb").read())
        if not words:
            raise ValueError("-%s: the word list holds no word" % name)
        return words
    out, i = [], 0
    while i < len(spec):
        c = spec[i:i + 1]
        if c == b"?":
            i += 1
            x = spec[i:i + 1].decode("latin-1")
            if x != "?" and x not in GEN_CLASSES:
                raise ValueError("-%s: unknown class ?%s" % (name, x))
            c = b"?" if x == "?" else GEN_CLASSES[x]
        for b in c:
            if bytes([b]) in out:
                raise ValueError("-%s: the byte %r is in the set twice" % (name, chr(b)))
            out.append(bytes([b]))
        i += 1
    if not out:
        raise ValueError("-%s: the set is empty" % name)
    return out


def parse_mask(mask, custom=None):
    """the command line's -mask (and custom = {1: set, ...}: a set's text as -1 ... -4 takes it, or a list of bytes objects) -> positions"""
    mask = mask.encode("latin-1") if isinstance(mask, str) else bytes(mask)
    sets = {int(k): (list(v) if isinstance(v, (list, tuple)) else _brain_set(v, k)) for k, v in (custom or {}).items()}
    positions, run, i = [], b"", 0

    def flush():
        nonlocal run
        if run:
            positions.append([run])
            run = b""

    while i < len(mask):
        c = mask[i:i + 1]
        if c != b"?" or mask[i + 1:i + 2] == b"?":
            if c == b"?":
                i += 1
            if len(run) == GEN_ALT_LEN_MAX:
                flush()
            run += mask[i:i + 1]
            i += 1
            continue
        x = mask[i + 1:i + 2].decode("latin-1")
        flush()
        if x in ("1", "2", "3", "4"):
            if int(x) not in sets:
                raise ValueError("invalid -mask: ?%s needs -%s <set>" % (x, x))
            positions.append(list(sets[int(x)]))
        elif x in GEN_CLASSES:
            positions.append([bytes([b]) for b in GEN_CLASSES[x]])
        else:
            raise ValueError("invalid -mask: unknown class ?%s" % x)
        i += 2
    flush()
    if not positions:
        raise ValueError("invalid -mask: the template is empty")
    brain_count(positions)
    return positions


def brain_count(positions):
    """T, the number of candidates; ValueError for a template outside the format's limits"""
    if not 1 <= len(positions) <= GEN_POS_MAX:
        raise ValueError("invalid -mask: more than 16 positions" if positions else "a template has 1 ... 16 positions")
    if any(not p for p in positions) or any(len(a) > GEN_ALT_LEN_MAX for p in positions for a in p):
        raise ValueError("a position has at least one alternative, an alternative at most 255 bytes")
    if sum(max(len(a) for a in p) for p in positions) > GEN_L_MAX:
        raise ValueError("the template's candidates are longer than 256 bytes")
    if sum(len(p) for p in positions) > GEN_NALT_MAX or sum(len(a) for p in positions for a in p) > GEN_POOL_MAX:
        raise ValueError("a template has at most 2^22 alternatives and 2^28 bytes of them")
    T = 1
    for p in positions:
        T *= len(p)
    if T >= 1 << 64:
        raise ValueError("the template has 2^64 candidates or more")
    return T


def brain_table(positions):
    """positions -> the packed blob of include/ecloop_hip.h (ECL_GEN): header, pos[], alt[], pool"""
    brain_count(positions)
    pos, alt, pool, first = b"", b"", b"", 0
    for p in positions:
        pos += len(p).to_bytes(4, "little") + first.to_bytes(4, "little")
        first += len(p)
        for a in p:
            alt += len(pool).to_bytes(4, "little") + len(a).to_bytes(4, "little")
            pool += bytes(a)
    return b"GEN\0" + bytes([len(positions), 0, 0, 0]) + first.to_bytes(4, "little") + len(pool).to_bytes(4, "little") + pos + alt + pool


def brain_positions(blob):
    """the packed blob -> positions (what brain_table packed)"""
    blob = bytes(blob)
    if blob[:4] != b"GEN\0" or len(blob) < 16:
        raise ValueError("not a template")
    npos, nalt, pool_bytes = blob[4], int.from_bytes(blob[8:12], "little"), int.from_bytes(blob[12:16], "little")
    u32 = lambda at: int.from_bytes(blob[at:at + 4], "little")
    alt_at, pool_at = 16 + 8 * npos, 16 + 8 * npos + 8 * nalt
    if len(blob) != pool_at + pool_bytes:
        raise ValueError("not a template")
    return [[blob[pool_at + u32(alt_at + 8 * a): pool_at + u32(alt_at + 8 * a) + u32(alt_at + 8 * a + 4)] for a in range(u32(16 + 8 * p + 4), u32(16 + 8 * p + 4) + u32(16 + 8 * p))]
            for p in range(npos)]


def brain_candidate(positions, i):
    """candidate i (bytes) of the template"""
    digits = []
    for p in reversed(positions):
        i, d = divmod(i, len(p))
        digits.append(d)
    if i:
        raise ValueError("the index is outside the template")
    return b"".join(p[d] for p, d in zip(positions, reversed(digits)))


class FoundRecord:
    __slots__ = ("label", "h160", "pk", "prefix", "address", "split", "path", "phrase")

    def __init__(self, label, h160, pk):
        self.label, self.h160, self.pk = label, h160, pk
        self.split = None  # a record of a split-key search: the image e; pk is then the PARTIAL key (splitkey_combine), its lines end with split:<e>
        self.address = ""  # a record of prefix_search: the address text, appended to its lines
        self.prefix = ""  # a verified pub record: "02" / "03", the first byte of the compressed key its line prints
        self.path, self.phrase = None, None  # a record of cmd_seed: the path's text and the phrase (bytes), appended to its lines

    def line(self):
        """outfile format of ctx_write_found (main.c:193-195)"""
        return "%s\t%s\t%064x" % (self.label, self.prefix + "".join("%08x" % int(w) for w in self.h160), self.pk) + ("\t" + self.address if self.address else "") + \
            ("" if self.split is None else "\tsplit:%d" % self.split) + ("" if self.path is None else "\t%s\t%s" % (self.path, self.phrase.decode("latin-1")))

    def stdout_line(self):
        """stdout format (main.c:187-189)"""
        return "%s: %s <- %064x" % (self.label, self.prefix + "".join("%08x" % int(w) for w in self.h160), self.pk) + (" " + self.address if self.address else "") + \
            ("" if self.split is None else " split:%d" % self.split) + ("" if self.path is None else " %s %s" % (self.path, self.phrase.decode("latin-1")))


def collect_records(call, dev, cap, short=None):
    """All records of one device call: the caller's half of the overflow protocol (include/ecloop_hip.h).  call(cap) makes the call with a
    buffer of `cap` records -> (records, total).  Where total > cap (dense filters only) the device kept up to max(cap, 2^20) records of
    the call and the rest is read from there; only if it kept fewer than the call produced is the call made again with a buffer that fits -
    or, for a caller that cannot repeat its call, EclError(short) raised."""
    while True:
        raw, total = call(cap)
        if total <= cap:
            return raw
        rest = dev.fetch_found(cap, total - cap)
        if len(rest) == total - cap:
            return np.concatenate([raw, rest])
        if short:
            raise EclError(short)
        cap = total


class KeySearch:
    """ctx_t + cmd_add / cmd_mul for one GPU."""

    def __init__(self, flt, device=0, a33=True, a65=False, endo=False, ord_offs=0, verify=True, launch_keys=1 << 32,
                 half_group=0, max_lanes=0, device_cls=None, p2sh=False, eth=False, tr=False, pub=False, prefix=False, origin=None, mask=False, kdf=None, bip39=False, gen=False):
        if pub:
            a33 = False  # public keys are searched alone (with or without the endomorphism)
        elif tr:
            a33 = False  # Taproot is searched alone and without the endomorphism (the context refuses anything beside it)
        elif eth:
            a33 = False  # eth is searched alone (any other type beside it: the context refuses)
        elif not (a33 or a65 or p2sh):
            a33 = True  # main.c:825-827
        self.flt, self.a33, self.a65, self.endo, self.offs, self.verify = flt, a33, a65, endo, ord_offs, verify
        self.p2sh = p2sh  # P2SH-P2WPKH (no reference counterpart): records labelled "p2sh"
        self.eth = eth  # Ethereum addresses (no reference counterpart either): records labelled "eth"
        self.tr = tr  # Taproot output keys (BIP341 / BIP86 key path): records labelled "p2tr", h160 = the leading 20 bytes of the key
        self.pub = pub  # public keys by x: records labelled "pub", h160 = the leading 20 bytes of x
        self.stride = 1 << ord_offs
        if kdf not in (None,) + KDF_NAMES:
            raise ValueError("kdf is None, 'sha256', 'keccak', 'sha3' or 'camp2'")
        self.kdf = None if kdf == "sha256" else kdf  # the hash of cmd_mul_raw (kdf_digest); None: SHA-256
        self.bip39 = bool(bip39)  # the context of cmd_seed: the lines of mul_batch_raw are BIP39 phrases
        if bip39 and self.kdf:  # ("sha256" is no kdf: None by now)
            raise ValueError("bip39 does not go with a kdf")
        self.gen = bool(gen)  # the context of cmd_brain: the lines of mul_batch_raw are generated on the device from a template
        if gen and (bip39 or prefix or mask):
            raise ValueError("gen does not go with bip39, prefix or mask")
        if origin is not None and not (prefix or mask):
            raise ValueError("an origin goes with the prefix search only (prefix_search(origin=(x, y)))")
        # split-key search (prefix_search(origin=)): the walk is O + k G, the records' keys are partial keys
        self.origin = None if origin is None else (int(origin[0]), int(origin[1]))
        # device_cls: the GPU context (capi.Device); the CPU tests of the host logic pass a stand-in with the same surface, which need not know
        # the types it is not asked for: a flag is passed only when set.  prefix / mask: flt is a PrefixFilter / MaskFilter, whose table
        # stands where the bloom words stand (prefix_search)
        kw = {name: value for name, value in dict(p2sh=bool(p2sh), eth=bool(eth), tr=bool(tr), pub=bool(pub), prefix=bool(prefix), mask=bool(mask),
                                                  kdf=self.kdf, bip39=self.bip39, gen=self.gen, origin=origin is not None).items() if value}
        self.dev = (device_cls or Device)(device, a33=a33, a65=a65, endo=endo, ord_offs=ord_offs, **kw)
        if half_group or max_lanes:
            self.dev.set_geometry(half_group, max_lanes)
        if mask:
            self.dev.set_masks(flt.table)
        elif prefix:
            self.dev.set_prefixes(flt.table)
        else:
            self.dev.set_bloom(flt.words)
        if flt.hashes is not None:
            self.dev.set_list(flt.hashes)  # exact confirm on the device too (main.c:212-216); the host check stays
        self.launch_keys = launch_keys
        self.k_checked = 0
        self.k_found = 0
        self.found = []

    def close(self):
        self.dev.close()

    # label of a record -> the device method that re-derives its words from the key, and which of the method's results holds them
    # (p2sh: the script hash of that addr33 hash)
    _REDERIVE = {"addr33": ("verify", 0), "addr65": ("verify", 1), "p2sh": ("verify", 0), "eth": ("verify_eth", 0), "p2tr": ("verify_tr", 0),
                 "pub": ("verify_pub", 0)}

    def _verify(self, recs):
        """pk_verify_hash (main.c:248-263): re-derive the hits from their scalars - the hashes by the window-table sum, a public key by the
        double-and-add kernel, never the walk kernel (the self-test of the context pins the one against the other) - and compare the words.
        A p2tr / pub record holds the first 20 bytes of its key and leaves with all eight words of it, a pub record also with .prefix.
        With an origin (split-key search) image e of O + k G is O' + k' G: k' = the record's partial key, O' the same image of O."""
        groups = {}
        for r in recs:
            groups.setdefault(self._REDERIVE[r.label][0], []).append(r)
        for method, rs in groups.items():
            kw = {} if self.origin is None else {"origin": [splitkey_image_origin(self.origin, r.split) for r in rs]}
            *words, ok = getattr(self.dev, method)([r.pk for r in rs], **kw)
            hsh = self.dev.p2sh_hash(words[0]) if any(r.label == "p2sh" for r in rs) else None
            for i, r in enumerate(rs):
                want = [int(v) for v in (hsh[i] if r.label == "p2sh" else words[self._REDERIVE[r.label][1]][i])]
                if not ok[i] or want[:5] != [int(v) for v in r.h160[:5]]:
                    raise EclError("[!] error: hash mismatch (%s) pk: %064x" % (r.label, r.pk))
                if r.label in ("p2tr", "pub"):
                    r.h160 = want
                if r.label == "pub":
                    r.prefix = "%02x" % (2 | int(words[1][i]))

    def _collect(self, raw, key_of, verify, more=None):
        """the records of one device call that the list confirms -> FoundRecords with the key key_of(record) (more(found, record) sets a
        command's own fields), verified if `verify`, counted and added to .found"""
        recs = []
        for r in raw:
            if self.flt.confirm(r["h160"]):
                recs.append(FoundRecord(label_of(r["compressed"]), [int(v) for v in r["h160"]], key_of(r)))
                if more:
                    more(recs[-1], r)
        if verify:
            self._verify(recs)
        self.found.extend(recs)
        self.k_found += len(recs)
        return recs

    def _search_lines(self, call, n, cap, key_of, verify, more=None):
        """one device call of cmd_mul / cmd_mul_raw / cmd_seed over n lines (a dense filter, three types per line: the buffer may overflow)"""
        self._collect(collect_records(call, self.dev, max(cap, 2 * n)), key_of, verify, more)
        self.k_checked += n

    def add_keys(self, start, nkeys, cap=4096):
        """hash exactly nkeys keys from `start`, in launches of at most launch_keys keys"""
        b, lanes = self.dev.geometry()
        sweep = lanes * 2 * b  # launches that are whole sweeps keep every lane busy and continue without re-init
        per = max(sweep, self.launch_keys // sweep * sweep)
        kw = {} if self.origin is None else {"origin": self.origin}
        split = None if self.origin is None else lambda rec, r: setattr(rec, "split", int(r["endo"]))
        done = 0
        while done < nkeys:
            n = nkeys - done
            if n > self.launch_keys:  # what fits one launch goes as one call: the library then sizes the lanes to it
                n = min(n, per)
            s = (start + done * self.stride) % N
            raw = collect_records(lambda c: self.dev.add_range(s, n, cap=c, **kw), self.dev, cap)
            self._collect(raw, lambda r: calc_priv(s, self.stride, int(r["key_offset"]), int(r["endo"])), self.verify, split)
            done += n

    def cmd_add(self, range_s, range_e, rank=0, world=1):
        """reference semantics of `add -r A:B` (status counter included), the scan sharded over `world` GPUs"""
        job, njobs, hashed = job_plan(range_s, range_e, self.stride)
        lo, cnt = shard(hashed, rank, world)
        self.add_keys((range_s + lo * self.stride) % N, cnt)
        if rank == 0:
            self.k_checked += njobs * job * (6 if self.endo else 1)  # main.c:431
        return self.found

    def cmd_mul(self, scalars, cap=4096):
        """cmd_mul_worker body (main.c:530-535) for already parsed scalars"""
        chunk = 1 << 16
        for at in range(0, len(scalars), chunk):
            ks = scalars[at : at + chunk]
            # no verify: main.c:469,474 (a p2tr / pub record gets its whole key from the verification)
            self._search_lines(lambda c: self.dev.mul_batch(ks, cap=c), len(ks), cap, lambda r: ks[int(r["key_offset"])], (self.tr or self.pub) and self.verify)
        return self.found

    def cmd_mul_raw(self, lines, cap=4096):
        """`mul -raw [-kdf ...]` for lines of text (bytes objects): the device hashes them (Device.mul_batch_raw, with the hash the context
        was opened with); the key of a found line is its digest (kdf_digest, recomputed here), and every hit is re-derived from that key
        through the device - a device hash that disagrees with kdf_digest raises the hash mismatch error instead of reporting a wrong key"""
        chunk = 1 << 16
        for at in range(0, len(lines), chunk):
            part = lines[at : at + chunk]
            self._search_lines(lambda c: self.dev.mul_batch_raw(part, cap=c), len(part), cap,
                               lambda r: int.from_bytes(kdf_digest(self.kdf or "sha256", part[int(r["key_offset"])]), "big"), self.verify)
        return self.found

    def cmd_seed(self, phrases, paths, count=1, passphrase=b"", cap=4096):
        """`seed`: BIP39 phrases (bytes objects) x BIP32 paths (lists of elements or text), `count` consecutive values of each path's last
        element - on a KeySearch(bip39=True).  Per batch of 2^20 phrases one reuse = 0 call hashes the phrases, every further (path, index)
        walks from the kept master nodes.  The key of a found line is bip39_key's, recomputed here, and every hit is re-derived from it
        through the device: a device derivation that disagrees raises the hash mismatch error.  Records carry .path and .phrase."""
        if not self.bip39:
            raise ValueError("cmd_seed goes with KeySearch(bip39=True)")
        paths = [parse_path(p) if isinstance(p, str) else list(p) for p in paths]
        if not paths or not 1 <= count <= SEED_COUNT_MAX or (count > 1 and any(not p for p in paths)):
            raise ValueError("cmd_seed takes at least one path and a count of 1 ... 1024 (above 1: no path of depth 0)")
        todo = []
        for p in paths:
            last = p[-1] if p else 0
            if count > 1 and (last & (BIP32_HARDENED - 1)) + count > BIP32_HARDENED:
                raise ValueError("the last element of a path plus the count passes 2^31")
            todo += [p[:-1] + [last + j] for j in range(count)] if p else [p]
        for at in range(0, len(phrases), SEED_BATCH):
            part = phrases[at : at + SEED_BATCH]
            for i, path in enumerate(todo):
                def more(rec, r):
                    rec.path, rec.phrase = format_path(path), part[int(r["key_offset"])]
                self._search_lines(lambda c: self.dev.seed_batch(part, path, passphrase=passphrase, reuse=i > 0, cap=c), len(part), cap,
                                   lambda r: bip39_key(part[int(r["key_offset"])], path, passphrase), self.verify, more)
        return self.found

    def cmd_brain(self, mask, custom=None, first=0, last=None, cap=4096):
        """`brain`: the candidates first ... last (both included; default: all) of the template `mask` (text for parse_mask with `custom`,
        or positions) - on a KeySearch(gen=True), in calls of 2^24.  The phrase of a found line is brain_candidate's and its key that
        phrase's kdf_digest, both computed here, and every hit is re-derived from that key through the device: a generator that
        disagrees raises the hash mismatch error.  Records carry .path (the index in hex) and .phrase."""
        if not self.gen:
            raise ValueError("cmd_brain goes with KeySearch(gen=True)")
        positions = parse_mask(mask, custom) if isinstance(mask, (str, bytes)) else [list(p) for p in mask]
        T = brain_count(positions)
        last = T - 1 if last is None else last
        if not 0 <= first <= last < T:
            raise ValueError("first ... last lies in 0 ... T - 1 = %x" % (T - 1))
        blob = brain_table(positions)
        at = first
        while at <= last:
            n = min(BRAIN_CALL, last - at + 1)

            def more(rec, r):
                rec.path, rec.phrase = "%x" % (at + int(r["key_offset"])), brain_candidate(positions, at + int(r["key_offset"]))
            raw = collect_records(lambda c: self.dev.brain_batch(blob, at, n, cap=c), self.dev, cap)
            self._collect(raw, lambda r: int.from_bytes(kdf_digest(self.kdf or "sha256", brain_candidate(positions, at + int(r["key_offset"]))), "big"), self.verify, more)
            self.k_checked += n
            at += n
        return self.found


# ----------------------------------------------------------------------------------------------- prefix search (-p)
# The mirror of ecloop_amd/host/prefix_plan.h (the method is described there): patterns -> inclusive ranges over the 160-bit value, merged,
# with the patterns each range serves; and the address text of a hit.

B58_ALPHABET = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
BECH32_ALPHABET = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"
PREFIX_MAX_FRACTION_LOG2 = -16  # patterns that together cover more of the 160-bit space are refused
PREFIX_MAX_RANGES = 1 << 16


class PrefixError(ValueError):
    """a refused pattern; the text names the pattern and the reason"""


def _prefix_form(s):
    if s[:2] in ("0x", "0X"):
        return "hex"
    if s[:4] in ("bc1q", "BC1Q"):
        return "bech32"
    if s[:1] == "1":
        return "b58"
    return None


def _pattern_ranges(s, a33, a65, eth):
    def fail(reason):
        raise PrefixError("pattern '%s': %s" % (s, reason))

    def bits_range(v, bits):
        lo = v << (160 - bits)
        return [(lo, lo + (1 << (160 - bits)) - 1)]

    if not s or len(s) > 44:
        fail("no address can start with it (empty or too long)")
    form = _prefix_form(s)
    if form is None:
        if s[0] == "3":
            fail("P2SH patterns (3...) are not supported yet")
        if s[:4] in ("bc1p", "BC1P"):
            fail("Taproot patterns (bc1p...) are not supported yet")
        if all(c in "0123456789abcdefABCDEF" for c in s):
            fail("bare hex patterns are not supported yet (an Ethereum pattern starts with 0x)")
        fail("no address can start with it (patterns start with 1, bc1q or 0x)")
    if form == "hex":
        if not eth:
            fail("a 0x pattern needs -a e")
        d = s[2:]
        if not 1 <= len(d) <= 40:
            fail("no address can start with it (1 ... 40 hex digits after 0x)")
        if any(c not in "0123456789abcdefABCDEF" for c in d):
            fail("a character that is no hex digit")
        return bits_range(int(d, 16), 4 * len(d))
    if form == "bech32":
        if eth or not a33 or a65:
            fail("a bc1q pattern needs -a c (P2WPKH is the compressed key's hash alone)")
        d = s[4:]
        if not 1 <= len(d) <= 32:
            fail("no address can start with it (1 ... 32 characters after bc1q)")
        upper = s[0] == "B"
        if any(c.islower() if upper else c.isupper() for c in d):
            fail("mixed case (bech32 is lower case, or all upper case)")
        v = 0
        for c in d.lower():
            if c not in BECH32_ALPHABET:
                fail("a character outside the bech32 alphabet (it has no 1, b, i, o)")
            v = v * 32 + BECH32_ALPHABET.index(c)
        return bits_range(v, 5 * len(d))
    if eth or not (a33 or a65):
        fail("a 1... pattern needs -a c, u or cu")
    if any(c not in B58_ALPHABET for c in s):
        fail("a character outside the base58 alphabet (it has no 0, O, I, l)")
    k = len(s) - len(s.lstrip("1"))
    z, m = k - 1, len(s) - k
    if z > 20:
        fail("no address can start with it (more leading 1s than a hash has zero bytes)")
    if m == 0:
        return [(0, 0)] if z == 20 else bits_range(0, 8 * z)
    if m > 33:
        fail("no address can start with it (too long)")
    v = 0
    for c in s[k:]:
        v = v * 58 + B58_ALPHABET.index(c)
    L = 24 - z
    bmin, bmax = 1 << (8 * (L - 1)), (1 << (8 * L)) - 1
    out = []
    lo, hi1 = v, v + 1
    for _ in range(m, 34):
        if lo > bmax:
            break
        a, b = lo, hi1 - 1
        if b >= bmin:
            out.append((max(a, bmin) >> 32, min(b, bmax) >> 32))
        lo, hi1 = lo * 58, hi1 * 58
    if not out:
        fail("no address can start with it (no hash gives these leading digits)")
    return out


prefix_pattern_ranges = _pattern_ranges  # one pattern -> its (lo, hi) ranges before merging and before the 2^-16 bound (the tests' view)


def _words5(v):
    return [(v >> (32 * (4 - i))) & 0xFFFFFFFF for i in range(5)]


def prefix_ranges(patterns, a33=True, a65=False, eth=False):
    """-> (table, serves): the (n, 10) uint32 range table of Device.set_prefixes - lo[5], hi[5], most significant word first, sorted,
    disjoint - and per range the ascending list of the indices of the patterns it serves.  Raises PrefixError for a refused pattern."""
    patterns = list(patterns)
    if not patterns:
        raise PrefixError("no patterns given")
    items = sorted((lo, i, hi) for i, p in enumerate(patterns) for lo, hi in _pattern_ranges(p, a33, a65, eth))
    merged = []
    for lo, i, hi in items:
        if merged and lo <= merged[-1][1] + 1:
            merged[-1][1] = max(merged[-1][1], hi)
            merged[-1][2].add(i)
        else:
            merged.append([lo, hi, {i}])
    if sum(hi - lo + 1 for lo, hi, _ in merged) > 1 << (160 + PREFIX_MAX_FRACTION_LOG2):
        raise PrefixError("the patterns ('%s'%s) cover more than 2^-16 of all addresses: one launch would report more records than the device keeps; lengthen the pattern"
                          % (patterns[0], ", ..." if len(patterns) > 1 else ""))
    if len(merged) > PREFIX_MAX_RANGES:
        raise PrefixError("the patterns need more than 65536 ranges")
    table = np.array([_words5(lo) + _words5(hi) for lo, hi, _ in merged], dtype=np.uint32).reshape(-1, 10)
    return table, [sorted(s) for _, _, s in merged]


def _h160_bytes(h160):
    return b"".join(int(w).to_bytes(4, "big") for w in h160)


def address_b58(h160):
    """base58check(00 || hash160): the P2PKH address"""
    import hashlib
    raw = b"\0" + _h160_bytes(h160)
    raw += hashlib.sha256(hashlib.sha256(raw).digest()).digest()[:4]
    v, s = int.from_bytes(raw, "big"), ""
    while v:
        v, r = divmod(v, 58)
        s = B58_ALPHABET[r] + s
    return "1" * (len(raw) - len(raw.lstrip(b"\0"))) + s


def address_bech32(h160):
    """BIP173: hrp bc, witness version 0, the 20-byte program (P2WPKH)"""
    v = int.from_bytes(_h160_bytes(h160), "big")
    data = [0] + [(v >> (5 * (31 - i))) & 31 for i in range(32)]
    chk = 1
    for x in [3, 3, 0, 2, 3] + data + [0] * 6:
        b = chk >> 25
        chk = (chk & 0x1FFFFFF) << 5 ^ x
        for j, g in enumerate((0x3B6A57B2, 0x26508E6D, 0x1EA119FA, 0x3D4233DD, 0x2A1462B3)):
            if (b >> j) & 1:
                chk ^= g
    chk ^= 1
    return "bc1" + "".join(BECH32_ALPHABET[d] for d in data + [(chk >> (5 * (5 - i))) & 31 for i in range(6)])


def address_eth(h160):
    return "0x" + _h160_bytes(h160).hex()


# ---- Ethereum patterns with wildcards and suffixes (0xdead*beef): the mirror of ecloop_amd/host/mask_plan.h (the grammar is written there)
MASK_MAX_ENTRIES = 16


def mask_is_masked(s):
    """a 0x pattern with ? or *: what sends a whole list to the mask table"""
    return _prefix_form(s) == "hex" and ("?" in s[2:] or "*" in s[2:])


def mask_pattern_entry(s, eth=True):
    """one pattern of a masked list -> (mask, value, digits): 160-bit integers and the number of hex digits the pattern fixes"""
    def fail(reason):
        raise PrefixError("pattern '%s': %s" % (s, reason))

    if not s or len(s) > 44:
        fail("no address can start with it (empty or too long)")
    if _prefix_form(s) != "hex":
        _pattern_ranges(s, False, False, eth)  # (the other forms fail the type check of -a e, or the line below)
        fail("a list with ? or * holds 0x patterns only")
    if not eth:
        fail("a 0x pattern needs -a e")
    d = s[2:]
    stars = 0
    for c in d:
        if c == "*":
            stars += 1
            if stars > 1:
                fail("more than one * (a pattern has one run of free digits at most)")
        elif c != "?" and c not in "0123456789abcdefABCDEF":
            fail("a character that is no hex digit")
    head, tail = d.split("*") if stars else (d, "")
    if not stars and not head:
        fail("no address can start with it (1 ... 40 hex digits after 0x)")
    if len(head) + len(tail) > 40:
        fail("no address can match it (too long: an address has 40 digits)")
    m = v = digits = 0
    for k, c in [(i, c) for i, c in enumerate(head)] + [(40 - len(tail) + j, c) for j, c in enumerate(tail)]:
        if c != "?":
            m |= 0xF << (4 * (39 - k))
            v |= int(c, 16) << (4 * (39 - k))
            digits += 1
    if not digits:
        fail("no hex digit at all: every address matches it")
    return m, v, digits


def mask_table(patterns, eth=True):
    """-> (table, serves): the (n, 10) uint32 mask table of Device.set_masks - m[5], v[5], most significant word first, the distinct entries
    in the order of their first pattern - and per entry the ascending list of the indices of the patterns it serves.  Raises PrefixError
    for a refused pattern, for more than 16 distinct entries and for a list whose entries together may cover more than 2^-16 of the space"""
    from fractions import Fraction
    patterns = list(patterns)
    if not patterns:
        raise PrefixError("no patterns given")
    entries, serves, total = [], [], Fraction(0)
    for i, p in enumerate(patterns):
        m, v, digits = mask_pattern_entry(p, eth)
        if (m, v) in entries:
            serves[entries.index((m, v))].append(i)
            continue
        if len(entries) == MASK_MAX_ENTRIES:
            raise PrefixError("the patterns ('%s', ...) need more than 16 mask entries: split the list" % patterns[0])
        entries.append((m, v))
        serves.append([i])
        total += Fraction(1, 16 ** digits)
    if total > Fraction(2) ** PREFIX_MAX_FRACTION_LOG2:
        raise PrefixError("the patterns ('%s'%s) cover more than 2^-16 of all addresses: one launch would report more records than the device keeps; lengthen the pattern"
                          % (patterns[0], ", ..." if len(patterns) > 1 else ""))
    table = np.array([_words5(m) + _words5(v) for m, v in entries], dtype=np.uint32).reshape(-1, 10)
    return table, serves


def _hex_pattern_matches(p, a):
    """does the lower-case text a = 0x + 40 digits match the 0x pattern p: by the text, ? any digit, the part after a * at the end"""
    d = p[2:].lower()
    head, tail = d.split("*") if "*" in d else (d, "")
    body = a[2:]
    return len(head) + len(tail) <= 40 and all(c in ("?", body[i]) for i, c in enumerate(head)) and all(c in ("?", body[40 - len(tail) + j]) for j, c in enumerate(tail))


def prefix_match(patterns, h160, label):
    """the address text of a record in the form of the first pattern, in list order, that it starts with (a 0x pattern with ? or *: that
    it matches); None if there is none (a range's end value whose checksum does not fit).  label: the record's (addr33, addr65, eth)"""
    for p in patterns:
        form = _prefix_form(p)
        if form == "hex" and label == "eth":
            a = address_eth(h160)
            if _hex_pattern_matches(p, a):
                return a
        elif form == "bech32" and label == "addr33":
            a = address_bech32(h160)
            a = a.upper() if p[0] == "B" else a
            if a.startswith(p):
                return a
        elif form == "b58" and label in ("addr33", "addr65"):
            a = address_b58(h160)
            if a.startswith(p):
                return a
    return None


class MaskFilter:
    """what KeySearch takes in place of a Filter for a search of masked Ethereum patterns: the mask table"""

    def __init__(self, table):
        self.table, self.words, self.hashes = table, None, None

    def confirm(self, h160):
        return True


class PrefixFilter:
    """what KeySearch takes in place of a Filter for a prefix search: the range table; every record the device reports counts"""

    def __init__(self, table):
        self.table, self.words, self.hashes = table, None, None

    def confirm(self, h160):
        return True


SPLITKEY_BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE  # x -> beta x is the point map of k -> lambda k


def splitkey_image_origin(origin, e):
    """image e (0 ... 5, the `endo` byte of a record) of the point (x, y): x times beta^(e // 2), y negated for odd e (host/splitkey.h)"""
    x, y = origin
    return x * pow(SPLITKEY_BETA, e // 2, P) % P, (P - y) % P if e & 1 else y


def splitkey_combine(kq, partial, e=0):
    """the requester's final key of a split-key hit: calc_priv(k_Q, e) + partial (mod n); e = 0: k_Q + partial (host/splitkey.h: sk_combine)"""
    return (calc_priv(kq % N, 1, 0, e) + partial) % N


def prefix_search(patterns, range_s, range_e, a33=True, a65=False, eth=False, endo=False, device=0, device_cls=None, verify=True, origin=None, **kw):
    """`add -p` for one GPU: the keys of [range_s, range_e) (cmd_add's job arithmetic) whose address starts with one of the patterns.
    -> (records, edge): FoundRecord objects with .address set, and the number of records dropped because their text matched no pattern.
    origin=(x, y), a point Q of the curve: the split-key search (`-p` with `-k`) - the walk is Q + k G, a record's pk is the PARTIAL key
    k' and .split the image e it belongs to: the address is that of the key splitkey_combine(k_Q, k', e), which only Q's owner can form"""
    patterns = list(patterns)
    if eth:
        a33 = a65 = False
    masked = any(mask_is_masked(p) for p in patterns)  # a list with a ? or * pattern becomes one mask table; any other is planned as ever
    if masked:
        flt, how = MaskFilter(mask_table(patterns, eth)[0]), {"mask": True}
    else:
        flt, how = PrefixFilter(prefix_ranges(patterns, a33, a65, eth)[0]), {"prefix": True}
    ks = KeySearch(flt, device=device, a33=a33, a65=a65, endo=endo, eth=eth, verify=verify, device_cls=device_cls, **how,
                   **({"origin": bsgs_point(origin)} if origin is not None else {}), **kw)
    try:
        out, edge = [], 0
        for r in ks.cmd_add(range_s, range_e):
            r.address = prefix_match(patterns, r.h160, r.label)
            if r.address is None and masked:  # the mask test is exact: no edges
                raise EclError("[!] error: the record %s matches no pattern" % address_eth(r.h160))
            if r.address is None:
                edge += 1
            else:
                out.append(r)
        return out, edge
    finally:
        ks.close()


def blf_gen(hashes, n, existing=None, device=0):
    """blf-gen (lib/utils.c:409-475): bloom of blf_size_words(n) words holding `hashes`; bulk insert on the GPU."""
    size = blf_size_words(n)
    words = np.zeros(size, dtype=np.uint64) if existing is None else np.ascontiguousarray(existing, dtype=np.uint64)
    if len(words) != size:
        raise ValueError("bloom filter size mismatch (%d != %d)" % (len(words), size))
    d = Device(device)
    try:
        d.set_bloom(words)
        d.bloom_insert(hashes)
        return d.get_bloom(size)
    finally:
        d.close()


# ----------------------------------------------------------------------------------------------- bsgs: the key of a known public key


def bsgs_plan(a, b, beta):
    """the arithmetic of host/bsgs_plan.h in Python integers (the method is written there): h = 2^beta baby steps, s = 2h keys per giant
    step, N = ceil((b - a + 1) / s) steps W_i = (2a + s - 1 + 2s i) G - 2Q; ranges with 2 (b + s) + 1 >= n are refused"""
    if not (0 <= beta <= 62) or a < 1 or a > b or b >= N:
        raise ValueError("bsgs: the range must satisfy 1 <= a <= b < n")
    h, s = 1 << beta, 2 << beta
    if 2 * (b + s) + 1 >= N:
        raise ValueError("bsgs: the range reaches n / 2 (2 (b + s) + 1 >= n): a giant step could be the point at infinity")
    return {"beta": beta, "h": h, "s": s, "steps": (b - a + s) // s, "baby_start": 1, "baby_offs": 1, "baby_keys": h,
            "giant_start": 2 * a + s - 1, "giant_offs": beta + 2, "filter_words": max(h, 1024)}


def bsgs_default_beta(a, b):
    return min(30, max(10, (b - a + 1).bit_length() // 2))  # ceil((bits - 1) / 2), clamped (unmeasured: tools/bench_bsgs.py)


def bsgs_point(pub):
    """a public key as 66 hex digits (02 / 03) or 130 (04, checked on the curve), or an (x, y) pair -> (x, y); a bare x names two keys
    and is refused"""
    if isinstance(pub, (tuple, list)):
        x, y = int(pub[0]), int(pub[1])
    else:
        t = pub.strip().lower()
        if len(t) == 66 and t[:2] in ("02", "03"):
            x = int(t[2:], 16)
            y = pow((x ** 3 + 7) % P, (P + 1) // 4, P) if x < P else 0
            if (y & 1) != (t[1] == "3"):
                y = P - y
        elif len(t) == 130 and t[:2] == "04":
            x, y = int(t[2:66], 16), int(t[66:], 16)
        else:
            raise ValueError("bsgs: a public key is 66 hex digits (02.. / 03..) or 130 (04..); a bare x names two keys")
    if not (x < P and 0 < y < P and (y * y - x ** 3 - 7) % P == 0):
        raise ValueError("bsgs: the public key is not a point of the curve")
    return x, y


def bsgs_origin(q):
    """O = -2Q"""
    x, y = q
    lam = 3 * x * x * pow(2 * y, P - 2, P) % P
    x2 = (lam * lam - 2 * x) % P
    return x2, (-(lam * (x - x2) - y)) % P


def _words5_of_x(x):
    return [(x >> (32 * (7 - j))) & 0xFFFFFFFF for j in range(5)]


def bsgs_search(pub, range_s, range_e, baby_log2=None, filter_words=None, device=0, device_cls=None, cap=4096):
    """baby-step giant-step search for the key of `pub` in [range_s, range_e] on one GPU -> (key or None, stats); stats: baby_keys,
    giant_steps (walked), false_positives (giant steps whose window held no key), windows_rescanned.  The baby filter is built once by an
    insert context, copied into the origin context that walks the giant steps; a record names a window, which an ordinary public-key
    context rescans, and a key is accepted only if all of x and the parity of y of its point are the target's."""
    Dev = device_cls or Device
    q = bsgs_point(pub)
    beta = bsgs_default_beta(range_s, range_e) if baby_log2 is None else int(baby_log2)
    while True:
        plan = bsgs_plan(range_s, range_e, beta)
        nwords = int(filter_words) if filter_words else plan["filter_words"]
        ins = Dev(device, a33=False, pub=True, insert=True, ord_offs=plan["baby_offs"])
        try:
            try:
                ins.set_bloom(np.zeros(nwords, np.uint64))
            except (EclError, MemoryError):
                if baby_log2 is None and not filter_words and beta > 10:
                    beta -= 1  # the filter does not fit: fewer baby steps
                    continue
                raise
            _, total = ins.add_range(plan["baby_start"], plan["baby_keys"], cap=1)
            if total:
                raise EclError("bsgs: the insert walk reported records")
            words = ins.get_bloom(nwords)
        finally:
            ins.close()
        break
    stats = {"baby_keys": plan["baby_keys"], "giant_steps": 0, "false_positives": 0, "windows_rescanned": 0}
    h5 = _words5_of_x(q[0])
    giant = Dev(device, a33=False, pub=True, origin=True, ord_offs=plan["giant_offs"])
    scan = None
    try:
        giant.set_bloom(words)
        origin, done = bsgs_origin(q), 0
        while done < plan["steps"]:
            n = min(plan["steps"] - done, 1 << 32)
            start = plan["giant_start"] + (done << plan["giant_offs"])
            raw = collect_records(lambda c: giant.add_range(start, n, cap=c, origin=origin), giant, cap,
                                  short="bsgs: more records in one call than the device keeps; use a larger filter")
            stats["giant_steps"] += n
            for off in sorted(int(r["key_offset"]) for r in raw):
                first = range_s + (done + off) * plan["s"]
                nk = min(plan["s"], range_e - first + 1)
                if scan is None:
                    scan = Dev(device, a33=False, pub=True)
                    one = np.zeros(1024, np.uint64)
                    blf_add_host(one, np.array([h5], np.uint32))
                    scan.set_bloom(one)
                    scan.set_list(np.array([h5], np.uint32))
                    scan.set_lookahead(0)
                recs, _ = scan.add_range(first, nk, cap=64)
                stats["windows_rescanned"] += 1
                for r in sorted(int(r["key_offset"]) for r in recs):
                    key = first + r
                    x, par, ok = scan.verify_pub([key])
                    if ok[0] and sum(int(w) << (32 * (7 - j)) for j, w in enumerate(x[0])) == q[0] and int(par[0]) == (q[1] & 1):
                        return key, stats
                stats["false_positives"] += 1
            done += n
        return None, stats
    finally:
        giant.close()
        if scan is not None:
            scan.close()


# ----------------------------------------------------------------------------------------------- kangaroo: the same for wide ranges


def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def kangaroo_plan(a, b, herd_log2=None, dp_bits=None, seed=0):
    """the defaults of host/kangaroo_plan.h (kg_plan_make) in Python integers: from the range [a, b] the herd, the distinguished-point bits,
    the jump and spread bits, the base scalar of the tame herd and the steps of a round; the refusals as ValueError"""
    if a < 1 or a > b or b >= N:
        raise ValueError("kangaroo: the range must satisfy 1 <= a <= b < n")
    wbits = (b - a).bit_length()
    if wbits > 124:
        raise ValueError("kangaroo: the range holds more than 2^124 keys")
    if herd_log2 is not None and not 1 <= herd_log2 <= 24:
        raise ValueError("kangaroo: herd_log2 is 1 ... 24")
    if dp_bits is not None and not 0 <= dp_bits <= 32:
        raise ValueError("kangaroo: dp_bits is 0 ... 32")
    half = wbits // 2
    hl = herd_log2 if herd_log2 is not None else _clamp(half - 4, 1, 22)
    dp = dp_bits if dp_bits is not None else _clamp(max(half - hl - 1, half + 2 - 26), 0, 32)
    return {"wbits": wbits, "herd_log2": hl, "dp": dp, "jb": _clamp(half + hl - 2, 4, 120), "sb": _clamp(wbits, 1, 124),
            "round_steps": 1 << _clamp(min(half - 1 - hl, 34 - hl), 0, 33), "base": a, "seed": seed}


def kangaroo_give_up(plan, max_factor):
    """the give-up limit in jumps: max_factor * 2 sqrt(W) + H 2^dp, sqrt(W) taken as 2^ceil(wbits / 2)"""
    return (max_factor << (1 + (plan["wbits"] + 1) // 2)) + (1 << (plan["herd_log2"] + plan["dp"]))


def kangaroo_candidates(base, d_tame, d_wild):
    """the two keys a tame / wild pair with equal identity stands for"""
    return (base + d_tame - d_wild) % N, (-(base + d_tame) - d_wild) % N


def _dp_identity(r):
    return int(r["h160"][2]) << 64 | int(r["h160"][3]) << 32 | int(r["h160"][4])


def _dp_distance(r):
    return int(r["key_offset"]) | int(r["h160"][1]) << 64 | int(r["h160"][0]) << 96


def kangaroo_search(pub, a, b, herd_log2=None, dp_bits=None, seed=0, max_factor=64, device=0, device_cls=None, round_steps=None):
    """Pollard's lambda search for the key of `pub` in [a, b] on one GPU -> (key or None, stats); stats: jumps, rounds, dps (distinguished
    points stored), same_herd (collisions inside a herd: counted, not acted on), candidates_checked.  A round is one add_range of
    round_steps jumps per kangaroo on an ECL_PUB | ECL_HERD context; its records, sorted by (identity, distance, herd), go into a table
    keyed on the identity; a tame / wild pair gives two candidates, each re-derived by the double-and-add kernel and accepted only if all
    of x and the parity of y are the target's.  None once the jumps reach the give-up limit (host/kangaroo_plan.h has the method)."""
    Dev = device_cls or Device
    q = bsgs_point(pub)
    plan = kangaroo_plan(a, b, herd_log2, dp_bits, seed)
    H, steps = 1 << plan["herd_log2"], int(round_steps or plan["round_steps"])
    limit = kangaroo_give_up(plan, max_factor)
    block = (plan["base"], q, seed, plan["herd_log2"], plan["jb"], plan["sb"])
    stats = {"jumps": 0, "rounds": 0, "dps": 0, "same_herd": 0, "candidates_checked": 0}
    store = {}
    cap = max(4096, 2 * ((steps * H) >> plan["dp"]) + 4096)
    d = Dev(device, a33=False, pub=True, herd=True, ord_offs=plan["dp"])
    try:
        while True:
            raw = collect_records(lambda c: d.add_range(None, steps * H, cap=c, herd=block), d, cap,
                                  short="kangaroo: more records in one round than the device keeps; use more dp bits")
            stats["jumps"] += steps * H
            stats["rounds"] += 1
            for ident, dist, herd in sorted((_dp_identity(r), _dp_distance(r), int(r["endo"])) for r in raw):
                have = store.get(ident)
                if have is None:
                    store[ident] = (dist, herd)
                    stats["dps"] += 1
                elif have[1] == herd:
                    stats["same_herd"] += 1
                else:
                    tame, wild = (have[0], dist) if herd else (dist, have[0])
                    for k in kangaroo_candidates(plan["base"], tame, wild):
                        stats["candidates_checked"] += 1
                        x, par, ok = d.verify_pub([k])
                        if ok[0] and sum(int(w) << (32 * (7 - j)) for j, w in enumerate(x[0])) == q[0] and int(par[0]) == (q[1] & 1):
                            return k, stats
            if stats["jumps"] >= limit:
                return None, stats
    finally:
        d.close()
