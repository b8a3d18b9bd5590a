"""The late start of emit33_ypar_short's d stream (csrc/emit33.h) on the CPU: column 8 for its digit alone, then columns 13..16 started
with no carry-in, and one compare of column 14's truncated digit, >= 2^29 - F, that sends a key the exact way.

par33_host -late (csrc/tools/par33_host.cpp) compares, case by case, emit33_ypar with fe_parity(fe_sub(fe_mul(lam, b), Y)) and with the
parity of (lam b - Y) mod p in its own big-number arithmetic, at the magnitudes of the walk (lam 1, b 6, Y 1), and checks what the header
of emit33.h derives: column 14 lacks f <= 19; below the guard its digit is the true one less f and u_6, u_7 and the last carry are the
true ones; column 7 then comes out low by at most 64.  Its sets:
  11  2^22 seeded random operand sets, of which at most one in 2^12 may take the exact path (the share is printed);
  12  limbs 4..8 of both factors at 0 or the ceiling in all 1024 patterns: the skipped columns 9..12 at their largest (f reaches 18 or 19);
  13  at least 256 sets whose truncated digit lies in [2^29 - F, 2^29), all by the exact path, and at least 256 in
      [2^29 - 2 F, 2^29 - F), none by it;
  14  at least 64 sets on which the late start without its guard gives a wrong u_6 (the program asserts that it does).
Limbs 0 and 1 have no part in columns 13 and 14, so sets 13 and 14 are solved for (one modular inverse each) where the search of the default
mode walks limb 0.  Here the kept records are checked once more in Python integers: the parity, the side of the guard, the wrong u_6."""
import re

import numpy as np

import par33_cases as C
import par33_late_cases as L


def counts(text):
    m = re.search(r"late: set 11: (\d+) random cases, (\d+) by the exact path, (\d+) of them inside the guard on column 14", text)
    p = re.search(r"late: set 12: 1024 patterns of limbs 4\.\.8; column 14 lacks at most (\d+) so far, column 7 at most (\d+)", text)
    s = re.search(r"late: search: (\d+) inside the guard, (\d+) just below, (\d+) where the late start alone gives a wrong u_6", text)
    e = re.search(r"late: largest carry lacking in column 14 (\d+), in column 7 (\d+)", text)
    t = re.search(r"late: (\d+) cases ok, (\d+) by the short way, (\d+) by the exact path", text)
    assert m and p and s and e and t, text[-3000:]
    return [[int(v) for v in x.groups()] for x in (m, p, s, e, t)]


def test_every_set_agrees_with_the_full_product_and_with_big_numbers():
    rc, text, recs = L.run()
    assert rc == 0, text[-3000:]
    print(text)
    (n1, exact1, guarded1), (f12, e12), (inside, under, wrong), (f, e), (n, short, exact) = counts(text)
    assert n1 >= 1 << 22 and exact1 * 4096 <= n1 and guarded1 <= exact1
    assert 18 <= f12 <= 19 and f <= 19 and e12 <= e <= 64
    assert inside >= 256 and under >= 256 and wrong >= 64
    assert n == short + exact and n == n1 + 2048 + inside + under + wrong and short > 0 and exact >= inside + wrong
    s = recs["set"]
    assert (s == 11).sum() == 1024 and (s == 12).sum() == 2048 and (s == 13).sum() == inside + under and (s == 14).sum() == wrong
    assert (recs["path"][s == 13] == 1).sum() == inside and (recs["path"][s == 13] == 0).sum() == under  # each side of the guard by its path
    assert (recs["path"][s == 14] == 1).all()


def test_kept_records_in_python_integers():
    rc, text, recs = L.run()
    assert rc == 0, text[-3000:]
    lam, b, y = C.values(recs["lam"]), C.values(recs["b"]), C.values(recs["Y"])
    want = np.array([((l * m - v) % C.P) & 1 for l, m, v in zip(lam, b, y)], dtype=np.uint32)
    bad = np.nonzero(want != recs["par"])[0]
    assert not len(bad), (int(bad[0]), recs[bad[0]].tolist(), int(want[bad[0]]))
    # the guard, on the digit as Python integers give it: whoever is inside goes the exact way; set 13 lies on its two sides, set 14 at its top
    late = [L.d_digits(r["lam"], r["b"], L.K0) for r in recs]
    u5 = np.array([d[5] for d in late])
    assert (recs["path"][u5 >= (1 << 29) - L.F] == 1).all()
    s13, s14 = recs["set"] == 13, recs["set"] == 14
    assert (u5[s13] >= (1 << 29) - 2 * L.F).all() and ((u5[s13] >= (1 << 29) - L.F) == (recs["path"][s13] == 1)).all()
    assert (u5[s14] >= (1 << 29) - 2).all()
    # a wrong u_6 by the late start alone: all of set 14, and nowhere outside the guard
    full = [L.d_digits(r["lam"], r["b"], None) for r in recs]
    wrong6 = np.array([d[6] != t[6] for d, t in zip(late, full)])
    assert wrong6[s14].all() and not wrong6[u5 < (1 << 29) - L.F].any()
    same = ~wrong6
    lack = np.array([t[5] - d[5] for d, t in zip(late, full)])
    assert (lack[same] >= 0).all() and lack[same].max() <= 19 and all(d[7] == t[7] for d, t, ok in zip(late, full, same) if ok)
    # the magnitudes are the walk's, and limbs 4..8 reach their ceilings together
    top = (recs["lam"][:, 4:8] == (1 << 29) + 449).all(axis=1) & (recs["lam"][:, 8] == (1 << 24) + 449)
    top &= (recs["b"][:, 4:8] == 6 * ((1 << 29) + 449)).all(axis=1) & (recs["b"][:, 8] == 6 * ((1 << 24) + 449))
    assert top.any() and recs["lam"][:, :8].max() == (1 << 29) + 449 and recs["b"][:, :8].max() == 6 * ((1 << 29) + 449)
    assert recs["lam"][:, 8].max() == (1 << 24) + 449 and recs["b"][:, 8].max() == 6 * ((1 << 24) + 449) and recs["Y"][:, :8].max() <= (1 << 29) + 449
