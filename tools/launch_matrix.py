"""`rocprofv3 --kernel-trace -- python tools/launch_matrix.py`: ONE launch per cell of the launch
choice's table (csrc/launch_choice.h; tests/test_host.py::test_launch_choice_table) that
`transform_device` or a fused pipeline reaches, at the table's N and T.  The dispatches of two
builds (FRUITS_HIP_LIB) must agree in kernel name, grid, workgroup and LDS size, line for line:
the check that a change of the host side moved no launch."""
import os, sys
sys.path.insert(0, ".")
import torch
import fruits_amd as fr
from fruits_amd import _native as nat
import bench

W23, W11, W42 = fr.words.of_weight(2, dim=3), fr.words.of_weight(1, dim=1), fr.words.of_weight(4, dim=2)
# (words, N, T, environment, semiring)
MATERIALISED = (
    (W23, 512, 1024, {}, None), (W23, 1536, 1024, {}, None), (W23, 1537, 1024, {}, None),
    (W23, 2048, 1024, {}, None), (W23, 2304, 1024, {}, None), (W23, 3072, 1024, {}, None),
    (W23, 8192, 1024, {}, None), (W23, 2048, 512, {}, None), (W23, 8192, 512, {}, None),
    (W23, 2048, 384, {}, None), (W23, 8192, 256, {}, None), (W23, 16384, 128, {}, None),
    (W23, 2048, 1024, {"FRUITS_HIP_STATIC": "0"}, None), (W23, 4096, 1024, {"FRUITS_HIP_STATIC": "0"}, None),
    (W23, 64, 1024, {"FRUITS_HIP_STATIC": "0"}, None),
    (W23, 2048, 1024, {"FRUITS_HIP_DEBUG": "wt=0"}, None), (W23, 2048, 1024, {"FRUITS_HIP_DEBUG": "tail=0"}, None),
    (W23, 24, 1024, {"FRUITS_HIP_DEBUG": "tail=8"}, None), (W11, 24, 1024, {"FRUITS_HIP_DEBUG": "tail=8"}, None),
    (W23, 2048, 1024, {"FRUITS_HIP_DEBUG": "groups=2"}, None),
    (W42, 2048, 1024, {}, None), (W42, 512, 4096, {}, None),
    (W23, 8192, 1024, {}, fr.semiring.Arctic(argmax=True)),
)
# (words, dimensions, N, T, weighting, sieves): the generic fused kernels (no compiler in a trace)
FUSED = (
    (W42, 2, 2048, 1024, None, [fr.sieving.NPI, fr.sieving.END]),
    (fr.words.of_weight(6, dim=2), 2, 8192, 1024, None, [fr.sieving.NPI, fr.sieving.END]),
    (fr.words.of_weight(9, dim=1), 1, 8192, 4096, None, [fr.sieving.NPI, fr.sieving.END]),
    (W23, 3, 4096, 256, fr.iss.weighting.Indices(total=True), [fr.sieving.NPI, fr.sieving.END]),
)


def with_env(env, fn):
    os.environ.update(env)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for key in env:
            del os.environ[key]


for words, N, T, env, semi in MATERIALISED:
    kw = {} if semi is None else {"semiring": semi}
    iss = fr.ISS(words, mode=fr.ISSMode.EXTENDED, **kw)
    Xd = bench._device_batch(torch, (N, 3, T), 0)
    with_env(env, lambda: iss.transform_device(Xd))
    print(f"materialised {len(words)} words N={N} T={T} {env}", flush=True)
for words, D, N, T, weighting, sieves in FUSED:
    def fused():
        p = bench._Pipeline(torch, fr, nat, (N, D, T), words, weighting, sieves, n_fit=32)
        fn, _, _ = p.launch()
        fn()
    with_env({"FRUITS_HIP_JIT": "0"}, fused)
    print(f"fused {len(words)} words N={N} T={T}", flush=True)
