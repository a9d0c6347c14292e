"""Index-level CPU emulation of clip_glass_amd/csrc/conv_down64.hip (test infrastructure, no GPU): the persistent walk with its priming
steps, the two register sets requested two steps ahead, the carried raw rows, the vertical-pass image, the 8-slot operand ring, the skip
and output images and every padding / store mask, thread by thread with the kernel's own address formulas.  LDS and the carry are
poisoned with NaN at every priming point (the kernel finds stale data there), so an output that reads a slot its own column segment has
not written comes out NaN.  The formulas restate the kernel; a change there must be mirrored here."""
import numpy as np

from fir_ops_ref import fir4      # fma(b + c, 3/8, (a + d) / 8) in fp16, as built: the one copy of it

TW, CIN, COUT = 29, 64, 128
ROWB = 64 * 128
V_BYTES, A_BYTES, XS_BYTES, O_BYTES = 4 * ROWB, 8 * ROWB, 2 * 32 * 128, 2 * 32 * 256
T = np.arange(512)


def vaddr(row, col, cg):
    return row * ROWB + ((col ^ ((col >> 2) & 1)) << 7) + (cg << 4)


def aaddr(rslot, slot, lc):
    return rslot * ROWB + (slot << 7) + ((lc ^ ((slot >> 1) & 7)) << 4)


def oaddr(row, px, c16):
    return row * (32 * 256) + (px << 8) + ((c16 ^ (px & 15)) << 4)


def gate(R, Cin, Cout):
    return Cin == CIN and Cout == COUT and R >= 16 and R % 4 == 0 and R * R * Cin < (1 << 31)


class _Walk:
    def __init__(self, first, last, tiles_x, SY):
        self.SY, self.tiles_x = SY, tiles_x
        self.left, self.prime = last - first, 1
        per_img = tiles_x * SY
        self.b = first // per_img
        rem = first - self.b * per_img
        self.tx = rem // SY
        self.s = rem - self.tx * SY
        self.total = self.left + 1 + (self.s + self.left - 1) // SY

    def issue(self):
        b, tx = self.b, self.tx
        if self.prime:
            self.prime = 0
            return dict(b=b, tx=tx, s=self.s - 1, valid=0, prime=1)
        st = dict(b=b, tx=tx, s=self.s, valid=int(self.left > 0), prime=0)
        if self.left > 1:
            self.s += 1
            if self.s == self.SY:
                self.s, self.prime = 0, 1
                self.tx += 1
                if self.tx == self.tiles_x:
                    self.tx = 0
                    self.b += 1
        if self.left > 0:
            self.left -= 1
        return st


def dblock_down64(h, xs, w1, ws, b1, n_cus=256, stats=None):
    """h [B,R,R,64], xs [B,R/2,R/2,64] (fp16-representable), w1 [128,64,3,3], ws [128,64,1,1], b1 [128] -> (y [B,R/2,R/2,128] float32,
    store count per output vector).  Unwritten outputs stay NaN."""
    B, R = h.shape[0], h.shape[1]
    assert gate(R, h.shape[3], w1.shape[0])
    Ro = R // 2
    h = h.astype(np.float16)
    xs = xs.astype(np.float16)
    Wm = np.transpose(w1.astype(np.float16).astype(np.float32), (2, 3, 0, 1)).reshape(9, COUT, CIN)         # [tap][n][ci]
    Wk = (ws.reshape(COUT, CIN).astype(np.float16).astype(np.float32) * np.float32(0.70710678118654752440)).astype(np.float16).astype(np.float32)
    y = np.full((B, Ro, Ro, COUT), np.nan, np.float32)
    count = np.zeros((B, Ro, Ro, COUT // 8), np.int32)
    tiles_x, SY = (Ro + TW - 1) // TW, Ro // 2
    steps = B * tiles_x * SY
    per_block = (steps + n_cus - 1) // n_cus
    grid = (steps + per_block - 1) // per_block
    n_prime = 0
    for wg in range(grid):
        first = wg * per_block
        last = min(first + per_block, steps)
        walk = _Walk(first, last, tiles_x, SY)
        lds = np.full(((V_BYTES + A_BYTES + XS_BYTES + O_BYTES) // 16, 8), np.nan, np.float16)
        Vs, As, Xs, Os = 0, V_BYTES // 16, (V_BYTES + A_BYTES) // 16, (V_BYTES + A_BYTES + XS_BYTES) // 16
        carry = np.full((3, 512, 8), np.nan, np.float16)

        def issue():
            st = walk.issue()
            cg, cs = T & 7, T >> 3
            col = np.clip(2 * TW * st["tx"] - 2 + cs, 0, R - 1)
            a = np.empty((4, 512, 8), np.float16)
            for k in range(4):
                iy = min(max(4 * st["s"] + 2 + k, 0), R - 1)
                a[k] = h[st["b"], iy, col][np.arange(512)[:, None], (cg * 8)[:, None] + np.arange(8)]
            v = np.minimum(T, 2 * TW * 8 - 1)
            row = (v >= TW * 8).astype(int)
            rem = v - row * (TW * 8)
            yy = np.clip(2 * st["s"] + row, 0, Ro - 1)
            xx = np.minimum(TW * st["tx"] + (rem >> 3), Ro - 1)
            st["a"] = a
            st["x"] = xs[st["b"], yy, xx][np.arange(512)[:, None], ((rem & 7) * 8)[:, None] + np.arange(8)]
            return st

        def step(Rg):
            nonlocal carry, n_prime
            b, tx, s, valid = Rg["b"], Rg["tx"], Rg["s"], Rg["valid"]
            if Rg["prime"]:             # what the kernel finds here is stale: poison it
                lds[:] = np.nan
                carry[:] = np.nan
                n_prime += 1
            ox, oy = 2 * TW * tx - 2, 4 * s + 2
            cg, cs = T & 7, T >> 3
            a = Rg["a"].copy()
            if ox < 0 or ox + 64 > R or oy < 0 or oy + 4 > R:
                colok = (ox + cs >= 0) & (ox + cs < R)
                for k in range(4):
                    ok = colok & (0 <= oy + k < R)
                    a[k][~ok] = 0
            c0, c1, c2 = carry
            lds[Vs + vaddr(0, cs, cg) // 16] = fir4(c0, c1, c2, a[0])
            lds[Vs + vaddr(1, cs, cg) // 16] = fir4(c1, c2, a[0], a[1])
            lds[Vs + vaddr(2, cs, cg) // 16] = fir4(c2, a[0], a[1], a[2])
            lds[Vs + vaddr(3, cs, cg) // 16] = fir4(a[0], a[1], a[2], a[3])
            carry = np.stack([a[1], a[2], a[3]])
            tt = T[T < 2 * TW * 8]
            row = (tt >= TW * 8).astype(int)
            rem = tt - row * (TW * 8)
            lds[Xs + aaddr(0, row * 32 + (rem >> 3), rem & 7) // 16] = Rg["x"][tt]
            new = issue()
            # horizontal pass
            lane, wave = T & 63, T >> 6
            row, j, cg = wave >> 1, (wave & 1) * 8 + (lane >> 3), lane & 7
            m = j < 15
            row, j, cg = row[m], j[m], cg[m]
            v = [lds[Vs + vaddr(row, 4 * j + k, cg) // 16].copy() for k in range(7)]
            rslot = (4 * s + 1 + row) & 7
            for i in range(4):
                c = 4 * j + i
                slot = np.where(c & 1, 32 + (c >> 1), c >> 1)
                lds[As + aaddr(rslot, slot, cg) // 16] = fir4(v[i], v[i + 1], v[i + 2], v[i + 3])
            # MFMA phase: wave (r, nb), lane (lr, kh)
            lr = np.arange(32)
            for r in range(2):
                acc = np.zeros((32, COUT), np.float64)      # float64 sums (order-free), rounded to fp32 where the kernel's accumulator is read
                with np.errstate(invalid="ignore"):
                    for ky in range(3):
                        rs = (4 * s + 2 * r + ky) & 7
                        for kx in range(3):
                            slot = (32 if kx == 1 else (kx >> 1)) + lr
                            frag = np.concatenate([lds[As + aaddr(rs, slot, lc) // 16] for lc in range(8)], axis=1).astype(np.float64)   # [px][ci]
                            acc += frag @ Wm[ky * 3 + kx].astype(np.float64).T
                    acc = acc.astype(np.float32) + b1.astype(np.float32)[None]
                    acc = np.maximum(acc, np.float32(0.2) * acc).astype(np.float64)
                    frag = np.concatenate([lds[Xs + aaddr(0, r * 32 + lr, lc) // 16] for lc in range(8)], axis=1).astype(np.float64)
                    acc += frag @ Wk.astype(np.float64).T
                    acc = acc.astype(np.float32)
                out = acc.astype(np.float16)
                for c16 in range(16):
                    lds[Os + oaddr(r, lr, c16) // 16] = out[:, c16 * 8:(c16 + 1) * 8]
            if valid:
                npx = min(TW, Ro - TW * tx)
                for k in range(2):
                    v = T + 512 * k
                    row = (v >= TW * 16).astype(int)
                    rem = v - row * (TW * 16)
                    px, ch = rem >> 4, rem & 15
                    m = (v < 2 * TW * 16) & (px < npx)
                    row, px, ch = row[m], px[m], ch[m]
                    vals = lds[Os + oaddr(row, px, ch) // 16].astype(np.float32)
                    for q in range(8):
                        y[b, 2 * s + row, TW * tx + px, ch * 8 + q] = vals[:, q]
                    np.add.at(count, (b, 2 * s + row, TW * tx + px, ch), 1)
            return new

        r0 = issue()
        r1 = issue()
        for _ in range(0, walk.total, 2):
            r0 = step(r0)
            r1 = step(r1)
        assert walk.left == 0 and walk.prime == 0, "the loop count does not cover the range"
    if stats is not None:
        stats["primes"] = n_prime
        stats["grid"] = grid
        stats["per_block"] = per_block
    return y, count


def reference(h, xs, w1, ws, b1):
    """The same op computed directly (no tiles): vertical then horizontal fir4 in fp16 on the zero-padded map, then the convolutions in
    float64 on the fp16 operands."""
    B, R = h.shape[0], h.shape[1]
    Ro = R // 2
    hp = np.zeros((B, R + 4, R + 4, CIN), np.float16)
    hp[:, 2:R + 2, 2:R + 2] = h.astype(np.float16)
    v = fir4(hp[:, 0:R + 1], hp[:, 1:R + 2], hp[:, 2:R + 3], hp[:, 3:R + 4])
    hb = fir4(v[:, :, 0:R + 1], v[:, :, 1:R + 2], v[:, :, 2:R + 3], v[:, :, 3:R + 4]).astype(np.float64)
    Wm = w1.astype(np.float16).astype(np.float64)
    acc = np.zeros((B, Ro, Ro, COUT))
    for ky in range(3):
        for kx in range(3):
            acc += hb[:, ky:ky + R - 1:2, kx:kx + R - 1:2] @ Wm[:, :, ky, kx].T
    acc += b1.astype(np.float64)
    acc = np.maximum(acc, 0.2 * acc)
    Wk = (ws.reshape(COUT, CIN).astype(np.float16).astype(np.float32) * np.float32(0.70710678118654752440)).astype(np.float16).astype(np.float64)
    return acc + xs.astype(np.float16).astype(np.float64) @ Wk.T
