"""The static programs' write-through instances (WalkCfg::WT, walk_static_inst.hip), read from the
compiler's gfx950 assembly: every full-chunk 16-byte output store of the plain instance becomes a
buffer store with the chosen cache policy, one for one, and nothing else in the node sequence
changes its waits.  Needs hipcc, no GPU."""
import os
import re
import subprocess

import pytest

from fruits_amd import build

CSRC = os.path.join(os.path.dirname(build.__file__), "csrc")


def _kernels(prog, tmp_path):
    """{mangled name: assembly lines} of the static walk kernels of program `prog`."""
    try:
        cc = build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc is not installed")
    out = tmp_path / f"static_{prog}.s"
    cmd = [cc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
           f"-DSTATIC_PROG={prog}", "--cuda-device-only", "-S", "-x", "hip",
           os.path.join(CSRC, "walk_static_inst.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    kernels, cur = {}, None
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\S*iss_walk_static_kernel\S*):", line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
            continue
        if cur is not None and line.startswith(".Lfunc_end"):
            cur = None
        if cur is not None:
            cur.append(line.strip())
    return kernels


def _count(lines, pattern):
    return sum(1 for l in lines if re.match(pattern, l))


# (program, its groups, the policy suffix of its write-through instance's stores)
@pytest.mark.parametrize("prog,policy", [(15, "sc1"), (16, "nt sc1")])
def test_write_through_instance_stores(prog, policy, tmp_path):
    kernels = _kernels(prog, tmp_path)
    assert len(kernels) == 2, sorted(kernels)
    # the WT instance is the one whose WalkCfg carries a non-zero last argument
    wt_name = [n for n in kernels if re.search(r"Lb0ELb0ELb0ELi(16|18)E", n)]
    assert len(wt_name) == 1, sorted(kernels)
    wt = kernels[wt_name[0]]
    plain = kernels[next(n for n in kernels if n != wt_name[0])]

    assert _count(plain, r"buffer_store") == 0
    full = [l for l in wt if l.startswith("buffer_store_dwordx4")]
    assert full, "no buffer stores in the write-through instance"
    for l in full:
        bits = [t for t in l.split("offen", 1)[1].split() if not t.startswith("offset:")]
        assert " ".join(bits) == policy, l
    # every 16-byte store of a full chunk has its twin in the ragged-chunk path, which stays a
    # plain global store (the plain instance's count differs: the compiler merges part of its two
    # identical paths)
    g_wt = _count(wt, r"global_store_dwordx4")
    assert g_wt == len(full), (g_wt, len(full))
    assert _count(plain, r"global_store_dwordx4") >= len(full)
    assert all(" sc" not in l and not l.endswith(" nt")
               for l in wt if l.startswith("global_store"))
    # no extra full drains of the memory counter, and no waterfall loop for the descriptor
    assert _count(wt, r"s_waitcnt vmcnt\(0\)") == _count(plain, r"s_waitcnt vmcnt\(0\)")
    assert _count(wt, r"v_readfirstlane") == _count(plain, r"v_readfirstlane")


def test_two_group_programs_have_one_instance(tmp_path):
    """Two-group programs were not measured: they keep plain stores and a single instance."""
    kernels = _kernels(2, tmp_path)
    assert len(kernels) == 1
    assert _count(next(iter(kernels.values())), r"buffer_store") == 0
