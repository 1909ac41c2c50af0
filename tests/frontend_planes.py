"""numpy restatement of the 16-bit plane formats of csrc/s3_format.h (split2h / join2h: two fp16 planes; split3: three bf16 planes) and of the block-4
plane layout the prep launch writes (csrc/kernels.h B4_*: one dword per pixel and plane, low half img1, high half the warped img2).  s3_format.h is the
reference: tests/test_frontend_planes_cpu.py holds these functions against it bit for bit, tests/test_gpu_frontend_batch.py carries them to the GPU."""
import numpy as np

F16_SCALE = np.float32(4096.0)
F16_INV = np.float32(1.0 / 4096.0)


def _f32(v):
    return np.ascontiguousarray(v, dtype=np.float32)


def f32_to_f16_bits(v):
    """round to nearest even, subnormal results kept, >= 65520 -> infinity (f32_to_f16_rn)"""
    with np.errstate(over="ignore"):
        return _f32(v).astype(np.float16).view(np.uint16)


def f16_bits_to_f32(b):
    return np.ascontiguousarray(b, dtype=np.uint16).view(np.float16).astype(np.float32)


def f32_to_bf16_bits(v):
    """round to nearest even of finite values (f32_to_bf16_rn)"""
    u = _f32(v).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFFFFFF)
    return (u >> np.uint64(16)).astype(np.uint16)


def bf16_bits_to_f32(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def split2h(v):
    """a = A0 + A1 / 4096: A0 = f16(v), A1 = f16((v - A0) * 4096), the difference and the product in fp32"""
    v = _f32(v)
    a = f32_to_f16_bits(v)
    with np.errstate(over="ignore", invalid="ignore"):
        r = ((v - f16_bits_to_f32(a)).astype(np.float32) * F16_SCALE).astype(np.float32)
    return a, f32_to_f16_bits(r)


def join2h(a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        return (f16_bits_to_f32(a) + (f16_bits_to_f32(b) * F16_INV).astype(np.float32)).astype(np.float32)


def split3(v):
    """the 3-way bf16 split: each plane is the bf16 rounding of what the planes before it left (fp32 differences)"""
    v = _f32(v)
    a = f32_to_bf16_bits(v)
    r = (v - bf16_bits_to_f32(a)).astype(np.float32)
    b = f32_to_bf16_bits(r)
    r2 = (r - bf16_bits_to_f32(b)).astype(np.float32)
    return a, b, f32_to_bf16_bits(r2)


def join3(a, b, c):
    return ((bf16_bits_to_f32(a) + bf16_bits_to_f32(b)).astype(np.float32) + bf16_bits_to_f32(c)).astype(np.float32)


def split_np(v, n_planes):
    """the planes of a context's arithmetic mode: 2 -> split2h, 3 -> split3 (tuple of n_planes uint16 arrays)"""
    if n_planes == 2:
        return split2h(v)
    if n_planes == 3:
        return split3(v)
    raise ValueError("n_planes must be 2 (fp16 planes) or 3 (bf16 planes)")


def join_np(planes):
    return join2h(*planes) if len(planes) == 2 else join3(*planes)


def pack(lo, hi):
    """one pixel's dword of one plane: low half img1's plane value, high half the warped img2's"""
    return np.ascontiguousarray(lo, dtype=np.uint16).astype(np.uint32) | (np.ascontiguousarray(hi, dtype=np.uint16).astype(np.uint32) << np.uint32(16))


def expected_planes(x, n_planes):
    """x [n, 2, 224, 320] fp32 (channel 0 img1, channel 1 warped img2) -> (dwords [n_planes, n, 224, 320] uint32 of the interior of the block-4 planes,
    joined [n, 2, 224, 320] fp32: what the planes add up to)"""
    x = _f32(x)
    p0, p1 = split_np(x[:, 0], n_planes), split_np(x[:, 1], n_planes)
    dwords = np.stack([pack(a, b) for a, b in zip(p0, p1)])
    return dwords, np.stack([join_np(p0), join_np(p1)], axis=1)


def plane_test_values():
    """the fixed value list of the CPU test: zeros, every k / 255, fp16 and bf16 rounding ties, values below 2^-14 (fp16 subnormal planes), 1.0,
    seeded uniform [0, 1) values, and a few negative and > 1 values"""
    f = np.float32
    vals = [f(0.0), f(-0.0), f(1.0)]
    vals += list(np.arange(256, dtype=np.float32) / f(255.0))
    for e in (0, -1, -3, -7, -13):                                  # halfway between two fp16 values of the binade 2^e, even and odd neighbours
        for m in (1, 3, 5, 2047):
            vals.append(f(np.ldexp(1.0 + m * 2.0 ** -11, e)))
    for m in (1, 3, 5, 255):                                        # bf16 ties (8 significand bits)
        vals.append(f(1.0 + m * 2.0 ** -8))
        vals.append(f(np.ldexp(1.0 + m * 2.0 ** -8, -9)))
    vals += [f(np.ldexp(1.0, -25)), f(np.ldexp(3.0, -25)), f(np.ldexp(5.0, -25)), f(np.ldexp(1.0, -25) * (1 + 2.0 ** -20))]   # ties of fp16 subnormals
    vals += [f(np.ldexp(1.0, -14)), f(np.ldexp(1.0, -14) * (1 - 2.0 ** -12)), f(np.ldexp(1.0, -15)), f(np.ldexp(1.3, -20)), f(np.ldexp(1.0, -24)),
             f(np.ldexp(1.0, -26)), f(1e-7), f(1e-10), f(1e-30), f(1e-40)]
    rng = np.random.default_rng(77)
    vals += list(rng.random(512, dtype=np.float32))
    vals += list((rng.random(64, dtype=np.float32) * f(2.0 ** -14)).astype(np.float32))
    vals += [f(-0.5), f(-1.0 / 255.0), f(-3.0), f(-1e-6), f(1.5), f(3.7), f(5.0), f(100.25), f(1e4), f(-1e4), f(32767.99), f(65504.0)]
    return np.array(vals, np.float32)
