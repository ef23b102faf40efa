"""The LDS bank-conflict depth the transform of csrc/vnd_spectrum.hpp predicts for itself: every read and
write of every Stockham stage, for every nfft, under the bank rule of a wave64 LDS access - float32: 4-byte accesses, bank
(a / 4) mod 32, two groups of 32 lanes; float64: 8-byte reads on (a / 4) mod 64 in two groups of 32 lanes, 8-byte writes on
(a / 4) mod 32 in four groups of 16 lanes.  Prints the mean LDS cycles per lane group (1.00: conflict-free) with the pad of
the kernel (point e at e + 5 * (e >> 5)) and without one.  Pure arithmetic: no device.

    python tools/spectrum_banks.py
"""
def pad(e, m=5): return e + m * (e >> 5)
def cycles(addrs, size, kind):
    # addrs: element indices for 64 lanes
    tot = 0
    if size == 4: groups = [range(0,32), range(32,64)]; mod = 32
    elif kind == 'r': groups = [range(0,32), range(32,64)]; mod = 64
    else: groups = [range(16*i,16*i+16) for i in range(4)]; mod = 32
    for g in groups:
        per = {}
        for l in g:
            a = addrs[l]*size
            for w in range(size//4):
                per.setdefault(((a//4)+w) % mod, set()).add(a//4 + w)
        tot += max(len(v) for v in per.values())
    return tot, len(groups)
def stage_cycles(ln, shift, size):
    N = 1 << ln; out = []
    ns = 1
    res = {}
    if ln & 1:
        r = w = ri = wi = 0
        for wave in range(4):
            for u in range(4):
                lanes = [wave*64 + l + u*256 for l in range(64)]
                g = [b >> (ln-1) for b in lanes]; j = [b & (N//2-1) for b in lanes]
                for half in range(2):
                    c, i = cycles([pad((gg << ln) + jj + half*(N//2), shift) for gg, jj in zip(g, j)], size, 'r'); r += c; ri += i
                    c, i = cycles([pad((gg << ln) + 2*jj + half, shift) for gg, jj in zip(g, j)], size, 'w'); w += c; wi += i
        res['r2'] = (r/ri, w/wi); ns = 2
    while ns < N:
        r = w = ri = wi = 0
        q = N >> 2
        for wave in range(4):
            for u in range(2):
                lanes = [wave*64 + l + u*256 for l in range(64)]
                g = [b >> (ln-2) for b in lanes]; j = [b & (q-1) for b in lanes]; k = [jj & (ns-1) for jj in j]
                for rr in range(4):
                    c, i = cycles([pad((gg << ln) + jj + rr*q, shift) for gg, jj in zip(g, j)], size, 'r'); r += c; ri += i
                    c, i = cycles([pad((gg << ln) + ((jj-kk) << 2) + kk + rr*ns, shift) for gg, jj, kk in zip(g, j, k)], size, 'w'); w += c; wi += i
        res['ns%d' % ns] = (r/ri, w/wi); ns <<= 2
    return res


if __name__ == '__main__':
    for size in (4, 8):
        for m in (0, 5):
            print('float%d, pad %d per 32 points' % (8 * size, m))
            for nfft in (64, 128, 256, 512, 1024, 2048, 4096):
                res = stage_cycles((nfft // 2).bit_length() - 1, m, size)
                print('  nfft %4d  ' % nfft + '  '.join('%s read %.2f write %.2f' % (k, v[0], v[1]) for k, v in res.items()))
