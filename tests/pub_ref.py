"""The yardstick of the public-key search (-a x, ECL_PUB): pure Python on the oracle's points (orc.point_of).  The x of k G, the five
leading big-endian words that are probed, the three endomorphism images a key gives with -endo, and the compressed encoding of the found
line.  Shares nothing with the device code."""
import orc

BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE  # beta^3 = 1 (mod p)
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72  # lambda^3 = 1 (mod n): lambda (x, y) = (beta x, y)


def x_of(k):
    """x of k G, or None for k = 0 (mod n)"""
    k %= orc.N
    return None if k == 0 else orc.point_of(k)[0]


def words5(x):
    """the leading 20 bytes of a 32-byte x as five big-endian words (the h160_t convention)"""
    return [(x >> (32 * (7 - i))) & 0xFFFFFFFF for i in range(5)]


def h160_of(k):
    return tuple(words5(x_of(k)))


def calc_priv(k, endo):
    """the key of image `endo` of k (main.c:267-276): 0 k, 1 -k, 2 lambda k, 3 -lambda k, 4 lambda^2 k, 5 -lambda^2 k"""
    k %= orc.N
    k = k * pow(LAMBDA, endo // 2, orc.N) % orc.N
    return (orc.N - k) % orc.N if endo & 1 else k


def endo_images(k):
    """with -endo a walked key is probed three times: {endo: the five words of x, beta x, beta^2 x} for endo = 0, 2, 4 (a key and its
    negative share x, so these stand for all six images)"""
    x = x_of(k)
    return {0: tuple(words5(x)), 2: tuple(words5(BETA * x % orc.P)), 4: tuple(words5(BETA * BETA * x % orc.P))}


def compressed(k):
    """the 66 hex digits of the compressed public key of k"""
    x, y = orc.point_of(k % orc.N)
    return "%02x%064x" % (2 | (y & 1), x)


def found_line(k):
    return "pub: %s <- %064x" % (compressed(k), k % orc.N)
