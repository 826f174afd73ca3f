"""Host twin of gv_synth_bed (csrc/gv_kernels.hip:k_synth_bed): the seeded synthetic .bed recipe of SURVEY 8d
in integer-only arithmetic, so the device generator and this numpy one produce identical bytes.  Input
generation only -- no part of the hot path."""
import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def synth_bed(N, M, seed, miss_ppm=5000, S=0, ld_block=0, ld_ppm=0):
    """Returns M * ceil(N/4) bytes, marker-major PLINK 2-bit (no magic bytes), for global markers S..S+M.
    ld_block > 0: gv_synth_bed_ld (block-correlated columns)."""
    mbytes = (N + 3) // 4
    miss_thr = np.uint64((miss_ppm << 32) // 1000000)
    ld_thr = np.uint64(min((ld_ppm << 32) // 1000000, 0xFFFFFFFF))
    with np.errstate(over="ignore"):
        g = np.arange(S, S + M, dtype=np.uint64)
        hm = _splitmix64(np.uint64(seed) ^ (g * np.uint64(0xD1342543DE82EF95)))
        maf = np.uint64(3277) + hm % np.uint64(29491)
        qv = np.uint64(65536) - maf
        p0 = (qv * qv) & np.uint64(0xFFFFFFFF)
        p1 = (np.uint64(2) * maf * qv) & np.uint64(0xFFFFFFFF)
        base = _splitmix64(hm + np.uint64(0x632BE59BD9B4E019))
        if ld_block:
            lbase = _splitmix64(np.uint64(seed) ^ ((g // np.uint64(ld_block)) * np.uint64(0xA24BAED4963EE407)) ^
                                np.uint64(0x5851F42D4C957F2D))
        n = np.arange(N, dtype=np.uint64)
        out = np.zeros((M, mbytes * 4), dtype=np.uint8)
        step = max(1, (1 << 22) // max(N, 1))
        for m0 in range(0, M, step):
            m1 = min(M, m0 + step)
            r = _splitmix64(base[m0:m1, None] + n[None, :])
            u = r >> np.uint64(32)
            um = r & np.uint64(0xFFFFFFFF)
            if ld_block:
                rs = _splitmix64(r ^ np.uint64(0x9FB21C651E98DF25))
                lat = _splitmix64(lbase[m0:m1, None] + n[None, :]) >> np.uint64(32)
                u = np.where((rs >> np.uint64(32)) < ld_thr, lat, u)
            P0 = p0[m0:m1, None]
            P1 = p1[m0:m1, None]
            code = np.zeros(r.shape, dtype=np.uint8)             # geno 2 -> 00
            code[((u - P0) & np.uint64(0xFFFFFFFF)) < P1] = 2      # geno 1 -> 10
            code[u < P0] = 3                                       # geno 0 -> 11
            code[um < miss_thr] = 1                                # missing -> 01
            out[m0:m1, :N] = code
    c = out.reshape(M, mbytes, 4)
    packed = c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)
    return packed.astype(np.uint8).reshape(-1)


def write_bed(path, bed_bytes):
    with open(path, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(np.ascontiguousarray(bed_bytes, dtype=np.uint8).tobytes())


def synth_meth(N, M, seed, S=0):
    """Host twin of gv_synth_meth (csrc/gv_dense.hip:k_synth_meth): the M x N methylation matrix (marker-major float64) of global
    markers S..S+M.  value(g, n) = c_g 2^-12 + (u0 + u1 + u2 + u3) 2^-19 -- an 11-bit per-marker centre plus an Irwin-Hall sum of
    the four 16-bit fields of a per-entry hash; every value is a dyadic rational exact in fp64, so the two agree bit for bit."""
    out = np.empty((M, N), dtype=np.float64)
    with np.errstate(over="ignore"):
        g = np.arange(S, S + M, dtype=np.uint64)
        hm = _splitmix64(np.uint64(seed) ^ (g * np.uint64(0xD1342543DE82EF95)))
        base = _splitmix64(hm + np.uint64(0x632BE59BD9B4E019))
        centre = (hm >> np.uint64(53)).astype(np.float64) * 2.0 ** -12
        n = np.arange(N, dtype=np.uint64)
        f = np.uint64(0xFFFF)
        step = max(1, (1 << 22) // max(N, 1))
        for m0 in range(0, M, step):
            m1 = min(M, m0 + step)
            r = _splitmix64(base[m0:m1, None] + n[None, :])
            s = (r & f) + ((r >> np.uint64(16)) & f) + ((r >> np.uint64(32)) & f) + (r >> np.uint64(48))
            out[m0:m1] = centre[m0:m1, None] + s.astype(np.float64) * 2.0 ** -19
    return out


def synth_dosage(N, M, seed, bits, S=0):
    """Host twin of gv_synth_dosage (csrc/gv_dense.hip:k_synth_dosage): the M x N dosage codes (marker-major uint8 / uint16) of global
    markers S..S+M.  Genotype g in {0, 1, 2} from two allele draws at the marker's frequency (655 + h mod 32113) / 65536, about
    0.01-0.5, plus a jitter, the product of two 16-bit hash fields: code = g * 3 * 2^(bits-3) + (jitter >> (18 - bits)).  Integer
    arithmetic only: the two agree bit for bit."""
    if bits not in (8, 16):
        raise ValueError("synth_dosage: bits must be 8 or 16")
    out = np.empty((M, N), dtype=np.uint8 if bits == 8 else np.uint16)
    with np.errstate(over="ignore"):
        g = np.arange(S, S + M, dtype=np.uint64)
        hm = _splitmix64(np.uint64(seed) ^ (g * np.uint64(0xD1342543DE82EF95)))
        base = _splitmix64(hm + np.uint64(0x632BE59BD9B4E019))
        maf = np.uint64(655) + hm % np.uint64(32113)
        n = np.arange(N, dtype=np.uint64)
        f = np.uint64(0xFFFF)
        step = max(1, (1 << 22) // max(N, 1))
        for m0 in range(0, M, step):
            m1 = min(M, m0 + step)
            r = _splitmix64(base[m0:m1, None] + n[None, :])
            q = maf[m0:m1, None]
            geno = ((r & f) < q).astype(np.uint64) + (((r >> np.uint64(16)) & f) < q).astype(np.uint64)
            jit = (((r >> np.uint64(32)) & f) * (r >> np.uint64(48))) >> np.uint64(16)
            out[m0:m1] = (geno * np.uint64(3 << (bits - 3)) + (jit >> np.uint64(18 - bits))).astype(out.dtype)
    return out


def synth_dosage_ld(N, M, seed, bits, ld_block, ld_ppm, miss_ppm=0, S=0):
    """Host twin of gv_synth_dosage_ld: synth_dosage's constants with synth_bed's block latent.  The two allele draws (the two low
    16-bit fields) read the block's latent hash lat = splitmix64(lbase + n) where rs >> 32 < ld_ppm * 2^32 / 10^6, rs a second hash of
    the entry, and the entry's own hash r elsewhere; the jitter always comes from the high 32 bits of r; a code equal to the reserved
    one is clamped one below it; a third hash below miss_ppm * 2^32 / 10^6 puts the reserved code.  Integer arithmetic only: the two
    agree bit for bit."""
    if bits not in (8, 16):
        raise ValueError("synth_dosage_ld: bits must be 8 or 16")
    if not 0 <= miss_ppm <= 1000000 or not 0 <= ld_ppm <= 1000000 or ld_block < 1:
        raise ValueError("synth_dosage_ld: miss_ppm and ld_ppm must be within 0..1000000, ld_block at least 1")
    out = np.empty((M, N), dtype=np.uint8 if bits == 8 else np.uint16)
    reserved = np.uint64((1 << bits) - 1)
    miss_thr = np.uint64((miss_ppm << 32) // 1000000)
    ld_thr = np.uint64(min((ld_ppm << 32) // 1000000, 0xFFFFFFFF))
    with np.errstate(over="ignore"):
        g = np.arange(S, S + M, dtype=np.uint64)
        hm = _splitmix64(np.uint64(seed) ^ (g * np.uint64(0xD1342543DE82EF95)))
        base = _splitmix64(hm + np.uint64(0x632BE59BD9B4E019))
        maf = np.uint64(655) + hm % np.uint64(32113)
        lbase = _splitmix64(np.uint64(seed) ^ ((g // np.uint64(ld_block)) * np.uint64(0xA24BAED4963EE407)) ^
                            np.uint64(0x5851F42D4C957F2D))
        n = np.arange(N, dtype=np.uint64)
        f = np.uint64(0xFFFF)
        step = max(1, (1 << 22) // max(N, 1))
        for m0 in range(0, M, step):
            m1 = min(M, m0 + step)
            r = _splitmix64(base[m0:m1, None] + n[None, :])
            rs = _splitmix64(r ^ np.uint64(0x9FB21C651E98DF25))
            lat = _splitmix64(lbase[m0:m1, None] + n[None, :])
            al = np.where((rs >> np.uint64(32)) < ld_thr, lat, r)
            q = maf[m0:m1, None]
            geno = ((al & f) < q).astype(np.uint64) + (((al >> np.uint64(16)) & f) < q).astype(np.uint64)
            jit = (((r >> np.uint64(32)) & f) * (r >> np.uint64(48))) >> np.uint64(16)
            code = geno * np.uint64(3 << (bits - 3)) + (jit >> np.uint64(18 - bits))
            code = np.minimum(code, reserved - np.uint64(1))
            code[(_splitmix64(rs ^ np.uint64(0x2545F4914F6CDD1D)) >> np.uint64(32)) < miss_thr] = reserved
            out[m0:m1] = code.astype(out.dtype)
    return out


def synth_dosage_na(N, M, seed, bits, miss_ppm, S=0):
    """Host twin of gv_synth_dosage_na: the codes of synth_dosage clamped one below the reserved code (255 / 65535), then, per entry,
    an independent draw -- the high 32 bits of a second hash of the entry below miss_ppm * 2^32 / 10^6 -- replaces the code by the
    reserved one.  Integer arithmetic only: the two agree bit for bit."""
    if not 0 <= miss_ppm <= 1000000:
        raise ValueError("synth_dosage_na: miss_ppm must be within 0..1000000")
    out = synth_dosage(N, M, seed, bits, S)
    reserved = (1 << bits) - 1
    out[out == reserved] = reserved - 1
    miss_thr = np.uint64((miss_ppm << 32) // 1000000)
    with np.errstate(over="ignore"):
        g = np.arange(S, S + M, dtype=np.uint64)
        hm = _splitmix64(np.uint64(seed) ^ (g * np.uint64(0xD1342543DE82EF95)))
        base = _splitmix64(hm + np.uint64(0x632BE59BD9B4E019))
        n = np.arange(N, dtype=np.uint64)
        step = max(1, (1 << 22) // max(N, 1))
        for m0 in range(0, M, step):
            m1 = min(M, m0 + step)
            r = _splitmix64(base[m0:m1, None] + n[None, :])
            rs = _splitmix64(r ^ np.uint64(0x9FB21C651E98DF25))
            out[m0:m1][(rs >> np.uint64(32)) < miss_thr] = reserved
    return out
