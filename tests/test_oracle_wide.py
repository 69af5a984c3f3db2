"""The oracle of each summation order at widths beyond 400 columns: Oracle(order=...) equals the reference's own loop
shape under the reference's flags (Probe(order=...)), bit for bit, so that the GPU tests of rows wider than 400 columns
compare against an order pinned to the reference at these widths too.  CPU only."""
import numpy as np
import pytest


def _host_has_fma():
    try:
        flags = open("/proc/cpuinfo").read()
    except OSError:
        return False
    return " avx2" in flags and " fma" in flags


# (the fma probe runs only on a host with AVX2 + FMA: elsewhere that order is not listed, rather than skipped)
ORDERS = ["sse2", "avx"] + (["fma"] if _host_has_fma() else [])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("D", [401, 402, 403, 404, 405, 406, 407, 408, 409, 415, 416, 512, 1000, 1031, 4099])
def test_oracle_matches_probe_at_wide_rows(order, D):
    from oracle.oracle import Oracle, Probe
    o, pr = Oracle(order=order), Probe(order=order)
    rng = np.random.default_rng(400 + D)
    c = (rng.normal(0, 1, (24, D)) * rng.choice([1e-3, 1.0, 50.0])).astype(np.float32)
    c[3] = c[7]                          # a duplicate: d2 = 0
    c[5] = c[2] + np.float32(1e-3)       # a close pair
    got = pr.pairwise_d2(c)
    full = np.array([[o.dist2(c[i], c[j]) if i != j else 0.0 for j in range(len(c))] for i in range(len(c))],
                    dtype=np.float32)
    np.fill_diagonal(got, 0.0)
    assert (bits(full) == bits(got)).all()
    assert (bits(got) == bits(got.T)).all()


@pytest.mark.parametrize("D", [408, 1000])
def test_orders_differ_at_wide_rows(D):
    """the orders are not copies of one another at these widths either"""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(D)
    c = rng.normal(0, 1, (32, D)).astype(np.float32)
    a, b = Oracle(order="sse2"), Oracle(order="avx")
    assert any(bits(a.dist2(c[0], c[j])) != bits(b.dist2(c[0], c[j])) for j in range(1, 32))
