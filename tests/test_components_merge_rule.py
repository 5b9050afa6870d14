"""The union rule of k_cc_rows / k_cc_merge (csrc/edt_components.hip) emulated sequentially: x-runs cut at every row start and at
every 256th voxel of the flattened volume, then, for every foreground voxel, the unions the kernel issues with the preceding
neighbour rows -- by the first voxel of an overlap only.  The components of exactly those unions must be the contract's
(tests/components_oracle.py): this holds the pruning and the index arithmetic, not the concurrency."""
import numpy as np
import pytest

import components_oracle as oracle

TILE = 256   # kCcTile


def emulate(lab, c, binary):
    sx, sy, sz = (lab.shape + (1, 1))[:3]
    L = lab.reshape(-1, order="F")
    n = L.size
    binary = binary or lab.dtype == np.bool_

    def fg(v):
        return v != 0

    def conn(a, b):
        return bool(fg(a) and fg(b)) if binary else bool(a == b and fg(a))

    P = [-1] * n
    for i in range(n):                                     # k_cc_rows
        if fg(L[i]):
            P[i] = P[i - 1] if i % sx != 0 and i % TILE != 0 and conn(L[i - 1], L[i]) else i

    def find(i):
        while P[i] != i:
            i = P[i]
        return i

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            P[max(a, b)] = min(a, b)

    def visit(p, v, q0, x, left, dilate):                  # cc_visit
        mc = conn(v, L[q0])
        if not dilate:
            if mc and not (left and conn(v, L[q0 - 1])):
                union(p, q0)
            return
        mr = x + 1 < sx and conn(v, L[q0 + 1])
        if left:
            if mr and not mc:
                union(p, q0 + 1)
            return
        if mc:
            union(p, q0)
            return
        if x > 0 and conn(v, L[q0 - 1]):
            union(p, q0 - 1)
        if mr:
            union(p, q0 + 1)

    sxy = sx * sy
    for p in range(n):                                     # k_cc_merge
        v = L[p]
        if not fg(v):
            continue
        row = p // sx
        x, z = p - row * sx, row // sy
        y = row - z * sy
        left = x > 0 and conn(L[p - 1], v)
        if left and p % TILE == 0:
            union(p, p - 1)
        if y > 0:
            visit(p, v, p - sx, x, left, c >= 2)
        if z > 0:
            visit(p, v, p - sxy, x, left, c >= 2)
            if c >= 2:
                if y > 0:
                    visit(p, v, p - sxy - sx, x, left, c >= 3)
                if y + 1 < sy:
                    visit(p, v, p - sxy + sx, x, left, c >= 3)
    out, number, k = np.zeros(n, dtype=np.uint32), {}, 0
    for i in range(n):                                     # roots in ascending order of index
        if P[i] == i:
            k += 1
            number[i] = k
    for i in range(n):
        if P[i] >= 0:
            out[i] = number[find(i)]
    return out.reshape(lab.shape, order="F"), k


@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_the_unions_the_kernel_issues_give_the_contracts_components(ndim):
    rng = np.random.default_rng(ndim)
    for trial in range(24):
        shape = {1: (int(rng.integers(1, 700)),), 2: (int(rng.integers(1, 300)), int(rng.integers(1, 12))),
                 3: (int(rng.integers(1, 280)), int(rng.integers(1, 7)), int(rng.integers(1, 5)))}[ndim]
        if trial % 3 == 0:    # long runs: the 256-voxel cut and the left-neighbour pruning
            lab = (rng.random(shape) < 0.85).astype(np.uint8) * rng.integers(1, 3, size=shape).astype(np.uint8)
        else:
            lab = rng.integers(0, int(rng.integers(2, 5)), size=shape).astype(np.uint8)
        lab = np.asfortranarray(lab)
        for c in range(1, ndim + 1):
            for binary in (False, True):
                got, gn = emulate(lab, c, binary)
                want, wn = oracle.connected_components(lab, c, binary=binary, return_N=True)
                assert gn == wn and np.array_equal(got, want), (shape, c, binary)
