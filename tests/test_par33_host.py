"""emit33_ypar (csrc/emit33.h) on the CPU: the parity of y = lam b - Y of a walked point from a partial product - fe_mul's d stream whole,
its c stream from column 6 on - against what it replaces and against big numbers.

The stand-alone program csrc/tools/par33_host.cpp compares, case by case, emit33_ypar with fe_parity(fe_sub(fe_mul(lam, b), Y)) and with
the parity of (lam b - Y) mod p in its own big-number arithmetic, at the magnitudes of the walk (lam 1, b 6, Y 1):
  1  2^22 seeded random operand sets, of which at most one in 2^12 may take the exact path (the guard costs 2^-16);
  2  limbs 5..8 of both factors at 0 or the ceiling in all 256 patterns;
  3  at least 256 sets whose truncated column 7 has its low 24 bits in [2^24 - G, 2^24), all by the exact path, and at least 256 in
     [2^24 - 2 G, 2^24 - G), none by it;
  4  at least 64 sets on which the short way without the guard gives the wrong parity (the program asserts that it does).
  5  four sets whose dropped carry crosses a multiple of 2^29 in column 7 while A is far from any boundary: only the guard sends them
     the exact way.  (The short value is still right on them unless limb 8 wraps too; the program prints how many it met.)
Here the records the program keeps are checked once more in Python integers, and the same program built with the address and
undefined-behaviour sanitizers has to run clean (its own main, nothing preloaded)."""
import re

import numpy as np

import par33_cases as C


def counts(text):
    m = re.search(r"set 1: (\d+) random cases, (\d+) by the exact path", text)
    s = re.search(r"search: (\d+) inside the guard, (\d+) just below, (\d+) where the short way alone is wrong; largest carry error (\d+)", text)
    t = re.search(r"par33_host: (\d+) cases ok, (\d+) by the short way, (\d+) by the exact path", text)
    assert m and s and t, text[-3000:]
    return [int(v) for v in m.groups()], [int(v) for v in s.groups()], [int(v) for v in t.groups()]


def check_run(rc, text, recs):
    assert rc == 0, text[-3000:]
    (n1, exact1), (inside, under, wrong, largest), (n, short, exact) = counts(text)
    print(text)
    assert n1 >= 1 << 22 and exact1 * 4096 <= n1
    assert inside >= 256 and under >= 256 and wrong >= 64 and largest <= 64
    assert n == short + exact and n >= n1 + 4096 + inside + under + wrong and short > 0 and exact >= inside + wrong
    s = recs["set"]
    assert (s == 1).sum() == 4096 and (s == 2).sum() == 4096 and (s == 3).sum() == inside + under and (s == 4).sum() == wrong
    assert (recs["path"][s == 3] == 1).sum() == inside and (recs["path"][s == 3] == 0).sum() == under  # each side of the guard by its path
    assert (recs["path"][s == 4] == 1).all()
    c = re.search(r"(\d+) sets whose dropped carry crosses 2\^29 in column 7 .*, (\d+) of them wrong by the short way", text)
    assert c and int(c.group(1)) >= 4 and (s == 5).sum() == int(c.group(1)) and (recs["path"][s == 5] == 1).all()


def test_every_set_agrees_with_the_full_product_and_with_big_numbers():
    check_run(*C.run())


def test_kept_records_in_python_integers():
    rc, text, recs = C.run()
    assert rc == 0, text[-3000:]
    lam, b, y = C.values(recs["lam"]), C.values(recs["b"]), C.values(recs["Y"])
    want = np.array([((l * m - v) % C.P) & 1 for l, m, v in zip(lam, b, y)], dtype=np.uint32)
    bad = np.nonzero(want != recs["par"])[0]
    assert not len(bad), (int(bad[0]), recs[bad[0]].tolist(), int(want[bad[0]]))
    # the magnitudes are the walk's: lam and Y at 1, b at 6, and the ceilings are reached
    assert recs["lam"][:, :8].max() == (1 << 29) + 449 and recs["b"][:, :8].max() == 6 * ((1 << 29) + 449)
    assert recs["lam"][:, 8].max() == (1 << 24) + 449 and recs["b"][:, 8].max() == 6 * ((1 << 24) + 449) and recs["Y"][:, :8].max() <= (1 << 29) + 449


def test_sanitizer_build_runs_clean():
    rc, text, recs = C.run(sanitize=True)
    check_run(rc, text, recs)
    assert "runtime error" not in text and "AddressSanitizer" not in text
    assert recs.tobytes() == C.run()[2].tobytes()  # the same cases, the same answers
