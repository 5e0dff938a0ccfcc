"""Byte rate of the float32 share of the substitution sweeps (k_cr_bwd, k_cr_fwd_off) from four runs of one build on one box: the bench command at the
default settings and with --lowp-switch 0 (fp64 throughout), each once under rocprofv3 --kernel-trace (scripts/rocpd_stats.py table, `steps` timed calls
incl. warm-up) and once under --pmc FETCH_SIZE alone (scripts/pmc_summary.py table, one step).
  float32 bytes B32  = bytes(k_cr_bwd, lowp 0) - bytes(k_cr_bwd, default): what reading the O blocks of the single-precision iterations as float32 removed,
                       i.e. the float32 bytes read (the same blocks are read once per sweep, so k_cr_fwd_off reads the same B32; its own byte difference
                       cannot be used: at the default settings it also runs the unfused pass-1 step of the float32 problems)
  fp64 rate    R64   = bytes / time of the kernel in the lowp 0 run
  float32 time t32   = time(default) - (bytes(default) - B32) / R64,   float32 rate = B32 / t32
FETCH_SIZE is in KiB and counts 128-byte requests as 64 B on gfx950 (scripts/pmc_traffic.py): bytes = 2 * 1024 * FETCH_SIZE.
usage: python scripts/subst_f32_rate.py <pmc default.txt> <pmc lowp0.txt> <kernel stats default.txt> <kernel stats lowp0.txt> [steps=3]"""
import sys


def pmc(path, kernel):
    for ln in open(path):
        if kernel + '(' in ln and 'FETCH_SIZE' in ln:
            f = ln.split()
            return 2.0 * 1024.0 * float(f[f.index('sum') + 1]), float(f[f.index('kernel_ms_total') + 1]), int(ln.split('n=')[1].split()[0])
    raise SystemExit(f'{kernel} not in {path}')


def kt(path, kernel, steps):
    for ln in open(path):
        if kernel + '(' in ln:
            f = ln[72:].split()
            return float(f[1]) / steps
    raise SystemExit(f'{kernel} not in {path}')


def main():
    pd, p0, kd, k0 = sys.argv[1:5]
    steps = int(sys.argv[5]) if len(sys.argv) > 5 else 3
    b32 = None
    print('%-14s %-9s %9s %9s %9s | %9s %9s %9s | %9s %9s %9s %8s' % ('kernel', 'setting', 'launches', 'GB/step', 'ms/step', 'fp64 TB/s', 'f32 GB', 'f32 ms', 'f32 TB/s', 'f32/fp64', 'fp64-eq ms', 'pmc ms'))
    for kernel in ('k_cr_bwd', 'k_cr_fwd_off'):
        bd, md, nd = pmc(pd, kernel); bl, ml, nl = pmc(p0, kernel)
        td, tl = kt(kd, kernel, steps), kt(k0, kernel, steps)
        if b32 is None:
            b32 = bl - bd
        r64 = bl / tl
        t32 = td - (bd - b32) / r64
        r32 = b32 / t32
        print('%-14s %-9s %9d %9.1f %9.2f | %9.3f' % (kernel, 'lowp 0', nl, bl / 1e9, tl, r64 / 1e9))
        print('%-14s %-9s %9d %9.1f %9.2f | %9s %9.1f %9.2f | %9.3f %9.3f %9.2f %8.2f' % (kernel, 'default', nd, bd / 1e9, td, '', b32 / 1e9, t32, r32 / 1e9, r32 / r64, 2 * b32 / r64, md))


if __name__ == '__main__':
    main()
