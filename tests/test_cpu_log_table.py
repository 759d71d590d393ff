"""The table log10 of the Brent objective (brent_core.h log10_mant_u, csrc/log_table.h) without a GPU: the committed
header is what tools/gen_log_table.py prints, byte for byte, and an exact-arithmetic emulation of log10_mant_u on the
header's own numbers -- every fma formed in fractions.Fraction and rounded once, the reference log10 in decimal at 60
digits -- keeps |z| < 2^-8 and the error bound of tests/native/num_check.hip's `log` section, 2^-53 + 1 ulp(|reference|),
over the table interval boundaries and random mantissas.  A table or series edit is caught here before it reaches a
device.  Standard library only."""
import math
import os
import random
import re
import subprocess
import sys
from decimal import Decimal, localcontext
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "polymutt_amd", "csrc", "log_table.h")
CORE = os.path.join(ROOT, "polymutt_amd", "csrc", "brent_core.h")
EXPONENTS = (0, -1, -340, -340000)
PREC = 60


def test_committed_table_is_the_generators_output():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_log_table.py")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(HEADER, "rb").read()


def _parse():
    text = open(HEADER).read()
    tab = [float.fromhex(v) for v in re.search(r"PM_LOG10_TAB_VALUES \{([^}]*)\}", text).group(1).split(",")]
    assert len(tab) == 256
    ser = [float.fromhex(re.search(rf"#define PM_LOG10_SER_{j} (\S+)", text).group(1)) for j in range(1, 7)]
    core = open(CORE).read()
    hi = float.fromhex(re.search(r"#define PM_LOG10_2_HI (\S+)", core).group(1))
    lo = float.fromhex(re.search(r"#define PM_LOG10_2_LO (\S+)", core).group(1))
    return tab, ser, hi, lo


def _rnd(q):
    """The double nearest a Fraction (int / int is correctly rounded)."""
    return q.numerator / q.denominator


def _fma(a, b, c):
    return _rnd(Fraction(a) * Fraction(b) + Fraction(c))


def _log10_mant_u(m, e, tab, ser, hi, lo):
    """brent_core.h log10_mant_u, operation for operation; returns (result, z)."""
    i = (int(math.ldexp(m, 53)) >> 45) & 0x7F   # the top 7 fraction bits: (hi word >> 13) & 0x7F
    c, L = tab[2 * i], tab[2 * i + 1]
    z = _fma(m, c, -1.0)
    p = _fma(z, ser[5], ser[4])
    for k in (3, 2, 1, 0):
        p = _fma(z, p, ser[k])
    de = float(e)
    tail = _rnd(Fraction(_rnd(Fraction(de) * Fraction(hi))) + Fraction(_rnd(Fraction(de) * Fraction(lo))))
    return _rnd(Fraction(_fma(z, p, L)) + Fraction(tail)), z


def _mantissas():
    out = [0.5, 1 - 2.0 ** -53]
    for i in range(129):   # four doubles on each side of every interval boundary 0.5 + i / 256 (1.0: below only)
        b = 0.5 + i / 256.0
        lo = hi = b
        for _ in range(4):
            lo = math.nextafter(lo, 0.0)
            if lo >= 0.5:
                out.append(lo)
            if hi < 1.0:
                out.append(hi)
            hi = math.nextafter(hi, 2.0)
    rng = random.Random(20240)
    out += [0.5 + rng.getrandbits(52) * 2.0 ** -53 for _ in range(2000)]
    return out


def test_exact_emulation_of_log10_mant_u_holds_the_bound():
    tab, ser, hi, lo = _parse()
    worst = {e: Decimal(0) for e in EXPONENTS}
    with localcontext() as ctx:
        ctx.prec = PREC
        ln10 = Decimal(10).ln()
        log2 = Decimal(2).ln() / ln10
        for m in _mantissas():
            assert 0.5 <= m < 1.0
            logm = Decimal(m).ln() / ln10   # Decimal(m) is the double, exactly
            for e in EXPONENTS:
                got, z = _log10_mant_u(m, e, tab, ser, hi, lo)
                assert abs(z) < 2.0 ** -8, (m.hex(), z)
                ref = logm + e * log2
                err = abs(Decimal(got) - ref)
                bound = Decimal(2.0 ** -53) + Decimal(math.ulp(abs(float(ref))))
                assert err <= bound, f"log10_mant_u({m.hex()}, {e}) = {got!r}, reference {ref}: error {err:.3E} > {bound:.3E}"
                worst[e] = max(worst[e], err)
    print("log10_mant_u exact emulation, max abs error per exponent:", {e: f"{float(v):.3g}" for e, v in worst.items()})
