// CPU check of the packed image's padded geometry for hidden widths that are
// multiples of 8 but not of 32: a layer with `in` inputs and `out` units is
// laid out in kt = ceil(in / 32) K-slices and nt = 2 * ceil(out / 32) 16-row
// tiles.  Over every element of those fragments drl::qnet_pack_slot (the pack
// kernel's element -> weight map) and drl::qnet_pack_elem (the learner's
// weight -> element map) must be mutual inverses on the real weights, every
// real weight must own exactly one element, and every other element must be a
// pad (row >= out or k outside [0, in)), which drl_qnet_pack writes as zero
// and the learner never writes.  Stand-alone host code: built and run by
// tests/test_narrow_nets.py, also under the address and undefined-behaviour
// sanitizers.
#include <stdio.h>

#include <vector>

#include "../../dronerl_amd/csrc/dronerl_internal.h"

// l: the layer's index in its net (>= 1: no policy-code K order); returns the number of violations
static int check(int l, int in, int out) {
    const int kt = (in + 31) / 32, nt = 2 * ((out + 31) / 32);
    const int64_t n = (int64_t)nt * kt * 512;
    std::vector<int> hits((size_t)out * in, 0);
    int bad = 0;
    int64_t pads = 0;
    for (int64_t e = 0; e < n; ++e) {
        const drl::PackSlot s = drl::qnet_pack_slot(l, e, kt, 0, in);
        if (s.row < 0 || s.row >= 16 * nt || s.k < 0 || s.k >= 32 * kt) ++bad;  // outside the physical layer
        const bool real = s.row < out && s.k >= 0 && s.k < in;
        if (!real) {
            ++pads;
            continue;
        }
        hits[(size_t)s.row * in + s.k]++;
        if (drl::qnet_pack_elem(l, s.row, s.k, kt, 0) != e) ++bad;  // elem(slot(e)) == e
    }
    for (int row = 0; row < out; ++row)
        for (int k = 0; k < in; ++k) {
            const int64_t e = drl::qnet_pack_elem(l, row, k, kt, 0);
            if (e < 0 || e >= n) {  // inside the layer's fragments
                ++bad;
                continue;
            }
            const drl::PackSlot s = drl::qnet_pack_slot(l, e, kt, 0, in);  // slot(elem(row, k)) == (row, k)
            if (s.row != row || s.k != k) ++bad;
            if (hits[(size_t)row * in + k] != 1) ++bad;  // exactly one element
        }
    if (pads != n - (int64_t)in * out) ++bad;  // every other element is a pad
    return bad;
}

int main() {
    const int ins[] = {8, 16, 24, 104}, outs[] = {8, 16, 24, 120};
    int total = 0;
    for (int l = 1; l <= 3; ++l)
        for (int in : ins)
            for (int out : outs) {
                const int b = check(l, in, out);
                if (l == 1 || b) printf("layer %d in %d out %d: %d bad\n", l, in, out, b);
                total += b;
            }
    printf(total ? "FAIL\n" : "OK\n");
    return total ? 1 : 0;
}
