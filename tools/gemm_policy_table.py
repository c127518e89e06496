"""The GEMM dispatch as a table: which kernel vst_gemm_kernel_name reports for every point of a fixed grid of
(M, N, K, kind, tile code, splits) and, at tile 0, of the settable knobs (8-phase tile width, persistent grid, conv
routing).  Host only: no GPU call beyond what loading the library does.

python tools/gemm_policy_table.py                 one `query -> name` line per grid point (about 430k lines)
python tools/gemm_policy_table.py --slice         the committed slice (tests/golden/gemm_policy.json's rows) as JSON lines
python tools/gemm_policy_table.py --rows FILE     the names this library gives for FILE's rows, one JSON list
python tools/gemm_policy_table.py --golden OUT --parent LIB
    writes OUT from the library LIB (a build of the parent commit); a row whose name differs in the in-tree library
    carries the in-tree name and the parent's as "was" (DESIGN.md lists the classes such rows may belong to)

VST_LIB_AB selects the library file, so two builds are compared with
    VST_LIB_AB=old/libvst_hip.so python tools/gemm_policy_table.py > old.txt; python tools/gemm_policy_table.py > new.txt
The VST_GEMM_* / VST_P8_* variables are read once per process by the library: run with them unset."""
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WS_BYTES = 80 << 20  # kernels._WS_BYTES
MS = (2, 8, 9, 300, 1024, 4096, 8192, 16562, 32768, 131072)
NS = (4, 32, 64, 128, 192, 320, 384, 512, 640, 1280, 1920, 2560, 10240)
KS = (96, 128, 320, 576, 640, 1152, 1280, 2880, 5120, 5760, 11520)
SPLITS = (0, 1, 3)
KNOBS = tuple(itertools.product((0, 192, 256, 320), (1, 0), (1, 0)))  # (p8 tile width, persist, conv)
DEFAULT = (0, 1, 1)
FIELDS = ("M", "N", "K", "kind", "tile", "splits", "bn", "persist", "conv")

# (M, N, K, kind) of every vst_gemm_ex / vst_conv3x3_ex launch of bench.py's denoise step (profiles/r6_shape_roofline.txt,
# r3s9_shapes.txt) and of the VAE (profiles/r6_vae_prof.txt, tools/vae_prof.py), at the default policy
WORKLOAD = [(m, n, k, 0) for m, n, k in (
    (131072, 320, 1280), (131072, 320, 320), (131072, 320, 640), (131072, 320, 960), (131072, 960, 320),
    (2, 1280, 1280), (2, 1280, 2816), (2, 1280, 320), (2, 13760, 1280), (32768, 1920, 640), (32768, 640, 1280),
    (32768, 640, 1920), (32768, 640, 2560), (32768, 640, 320), (32768, 640, 640), (32768, 640, 960),
    (8192, 1280, 1280), (8192, 1280, 1920), (8192, 1280, 2560), (8192, 1280, 5120), (8192, 1280, 640),
    (8192, 3840, 1280), (8192, 32, 1280), (32768, 32, 640), (262144, 256, 128), (4096, 512, 4096), (16384, 512, 512))]
WORKLOAD += [(m, n, k, 1) for m, n, k in ((131072, 2560, 320), (32768, 5120, 640), (8192, 10240, 1280))]
WORKLOAD += [(m, n, k, 2) for m, n, k in (
    (131072, 320, 2880), (131072, 320, 5760), (131072, 320, 8640), (131072, 4, 2880), (131072, 640, 5760),
    (32768, 1280, 11520), (32768, 320, 2880), (32768, 640, 11520), (32768, 640, 17280), (32768, 640, 2880),
    (32768, 640, 5760), (32768, 640, 8640), (8192, 1280, 11520), (8192, 1280, 17280), (8192, 1280, 23040),
    (8192, 1280, 5760), (8192, 640, 5760), (1048576, 128, 1152), (16384, 512, 4608), (262144, 128, 1152),
    (262144, 256, 1152), (262144, 256, 2304), (65536, 256, 2304), (65536, 512, 2304), (65536, 512, 4608),
    (1048576, 3, 1152))]
WORKLOAD += [(131072, 320, 40, 3), (1048576, 128, 32, 3)]
# forced tile codes: one small and one full-grid shape per kind
FORCED = ((300, 640, 1280, 0), (8192, 1280, 5120, 0), (300, 640, 1280, 1), (8192, 10240, 1280, 1),
          (300, 320, 2880, 2), (8192, 1280, 11520, 2), (300, 320, 40, 3), (131072, 320, 40, 3))
CROSSED = ((8192, 1280, 5120, 0), (32768, 640, 2560, 0), (8192, 10240, 1280, 1), (8192, 1280, 11520, 2),
           (65536, 512, 4608, 2))


def full_grid():
    for M, N, K, kind in itertools.product(MS, NS, KS, range(4)):
        if kind == 1 and N % 64:
            continue
        for tile, splits in itertools.product(range(11), SPLITS):
            for knobs in (KNOBS if tile == 0 else (DEFAULT,)):
                yield (M, N, K, kind, tile, splits) + knobs


def slice_rows():
    for shape in WORKLOAD:
        for splits in (1, 0):
            yield shape + (0, splits) + DEFAULT
    for shape, tile, splits in itertools.product(FORCED, range(1, 11), SPLITS):
        yield shape + (tile, splits) + DEFAULT
    for shape, splits, knobs in itertools.product(CROSSED, SPLITS, KNOBS):
        yield shape + (0, splits) + knobs


def names(rows):
    from video_style_transfer_amd import _lib
    lib = _lib.load()
    state = None
    for row in rows:
        if row[6:] != state:
            state = tuple(row[6:])
            lib.vst_p8_force_bn(state[0]), lib.vst_p8_persist(state[1]), lib.vst_p8_conv(state[2])
        yield (lib.vst_gemm_kernel_name(*row[:6], WS_BYTES) or b"").decode()


def read_rows(path):
    with open(path) as f:
        return json.load(f)


def child(args, lib=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("VST_GEMM_", "VST_P8_", "VST_LIB_AB"))}
    if lib:
        env["VST_LIB_AB"] = lib
    return subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, check=True,
                          capture_output=True, text=True).stdout


def main():
    a = sys.argv[1:]
    if a[:1] == ["--rows"]:
        print(json.dumps(list(names([tuple(r[f] for f in FIELDS) for r in read_rows(a[1])]))))
    elif a[:1] == ["--golden"]:
        old, new = (child(["--slice"], lib).splitlines() for lib in (a[a.index("--parent") + 1], None))
        rows = []
        for o, n in zip(old, new):
            o, n = json.loads(o), json.loads(n)
            if o["name"] != n["name"]:
                n["was"] = o["name"]
            rows.append(json.dumps(n))
        with open(a[1], "w") as f:  # one row per line
            f.write("[\n" + ",\n".join(rows) + "\n]\n")
    else:
        rows = list(slice_rows() if a[:1] == ["--slice"] else full_grid())
        for row, name in zip(rows, names(rows)):
            if a[:1] == ["--slice"]:
                print(json.dumps(dict(zip(FIELDS, row), name=name)))
            else:
                print(" ".join(f"{f}={v}" for f, v in zip(FIELDS, row)), "->", name)


if __name__ == "__main__":
    main()
