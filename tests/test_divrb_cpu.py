"""bm_div_rb of csrc/bmmath.hpp - y / b for a divisor that is the same in every lane, from the reciprocal the host formed once (the Normal
priors' (x - a) / b of the segment kernel's MH step) - must return the bits of the IEEE division for EVERY input: inside its admitted ranges
by Markstein's correction steps, outside them by taking `/` itself.  The header is compiled for the host (tests/divrb_check.c) and compared
with the host's division on 1e7 random pairs over the admitted exponent ranges, constructed hard cases (y = RN(b q) and its neighbours,
quotients at a binade edge, short mantissas that hit midpoints, powers of two), zeros / infinities / NaN, subnormal quotients, and both
ends of the admitted ranges with the doubles just outside them.  No mismatch is allowed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_div_rb_gives_the_bits_of_the_division(tmp_path):
    exe = str(tmp_path / "divrb_check")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "divrb_check.c"), "-lm"], check=True)
    r = subprocess.run([exe, "10000000"], capture_output=True, text=True)
    print(r.stdout)
    groups = dict((m.group(1), (int(m.group(2)), int(m.group(3)))) for m in re.finditer(r"^(\w+) (\d+) (\d+)$", r.stdout, re.M))
    for name in ("random", "random_near", "constructed", "short_mantissas", "binade_edge", "powers_of_two", "special_dividends",
                 "subnormal_quotients", "range_ends", "total"):
        assert name in groups, r.stdout
        tried, wrong = groups[name]
        assert tried > 0 and wrong == 0, (name, r.stdout)
    assert groups["random"][0] >= 10 ** 7
    assert r.returncode == 0, r.stdout
