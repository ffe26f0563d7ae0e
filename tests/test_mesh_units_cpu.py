"""The three mesh objects, each from a source of its own (hfcl_k_bvh.hip, hfcl_k_bvhc.hip, hfcl_k_bvhs.hip -> hfcl_k_bvh.o, hfcl_k_bvhc.o,
hfcl_k_bvhs.o), share templates (csrc/hfcl_mesh.hpp; the two collide() sources also csrc/hfcl_mesh_collide.hpp) and are built under two
contraction settings: a kernel instantiated with the same arguments in two of them would be built twice, differently, and meet at one
host stub.  Whatever two of them launch therefore carries the launching source's part (MESH_UNIT_PART) as a template argument.  Here:
the host stubs the built objects define are pairwise disjoint, each object defines its own number of them, and together they are the
60 kernels of the mesh units.  Symbol names only; no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hpp-fcl_amd", "csrc")
UNITS = ("hfcl_k_bvh.o", "hfcl_k_bvhc.o", "hfcl_k_bvhs.o")
KERNELS = {"hfcl_k_bvh.o": 19, "hfcl_k_bvhc.o": 27, "hfcl_k_bvhs.o": 14}  # (product build; profiles/r29_a_mesh_units.md section 1)


def defined_stubs(obj):
    """The __device_stub__ symbols the host object defines (one per kernel the unit launches)."""
    path = os.path.join(CSRC, obj)
    assert os.path.exists(path), "%s is not built: run `make -j16 -C hpp-fcl_amd/csrc`" % path
    if shutil.which("nm"):
        out = subprocess.run(["nm", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = [l.split()[-1] for l in out.splitlines() if l.strip()]
    else:  # ROCm's LLVM: Num Value Size Type Bind Vis Ndx Name
        out = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "--symbols", "--wide", path], capture_output=True, text=True, check=True).stdout
        rows = [l.split() for l in out.splitlines()]
        names = [r[7] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"]
    return {n for n in names if "__device_stub__" in n}


def test_no_kernel_is_built_in_two_mesh_units():
    stubs = {u: defined_stubs(u) for u in UNITS}
    for u in UNITS:
        assert stubs[u], u + " defines no kernel stub"
    for i, a in enumerate(UNITS):
        for b in UNITS[i + 1:]:
            both = stubs[a] & stubs[b]
            assert not both, "%s and %s both build %s: pass the unit's part to it (hfcl_mesh_collide.hpp)" % (a, b, sorted(both))
    counts = {u: len(stubs[u]) for u in UNITS}
    assert len(set().union(*stubs.values())) == 60, "kernels per mesh object: %s (stale objects? rebuild with make)" % counts
    # a kernel that drifts from one object into another (and so under another contraction setting) leaves the total at 60
    assert counts == KERNELS, "kernels per mesh object: %s, expected %s (stale objects? rebuild with make)" % (counts, KERNELS)
