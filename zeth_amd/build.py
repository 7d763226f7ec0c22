"""Build libzkhal_mi355x.so (gfx950) in-tree with hipcc, and the CPU oracle with gcc.

`python -m zeth_amd.build` or `__graft_entry__.build()`.  hipcc cross-compiles without a GPU.  The shared
library lands next to this file (git-ignored, but shipped to the GPU box by gpurun).
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)
# experiment builds of the same ABI (tools/gpu_*.sh A/B runs; loaded through ZKH_LIBRARY): ZKH_BUILD_VARIANT=<name>
# ZKH_BUILD_FLAGS="-D..." -> .variants/libzkhal_<name>.so with its own object directory
VARIANT = os.environ.get("ZKH_BUILD_VARIANT", "")
LIB = os.path.join(ROOT, ".variants", f"libzkhal_{VARIANT}.so") if VARIANT else os.path.join(HERE, "libzkhal_mi355x.so")
OBJ_DIR = os.path.join(ROOT, ".variants", f"_obj_{VARIANT}") if VARIANT else os.path.join(HERE, "csrc", "_obj")
SOURCES = ["hal.hip", "ntt.hip", "hash.hip", "poly.hip", "circuit.hip", "prover.hip", "verifier.hip", "session.hip", "recursion.hip", "topology.hip", "preflight.hip", "rec_builder.hip", "arguments.hip", "accumulate.hip", "multiplicities.hip", "sort.hip", "columns.hip", "links.hip", "page_out.hip", "image.hip", "page_circuit.hip", "page_tree.hip", "check_rows.hip", "bus.hip", "tie.hip"]   # + generated eval_check units
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-Wno-unused-result"] + os.environ.get("ZKH_BUILD_FLAGS", "").split()
# hash.hip: the unrolled Poseidon2 source order already interleaves 24 independent cells; LLVM's machine scheduler
# re-interleaves it up to the register budget (126 VGPRs instead of 86) for no measurable gain on MI355X (hash_rows
# M3 9.55 vs 9.59 ms): the source order is kept for the smaller footprint.
# accumulate.hip: the batch loops of k_args_terms must unroll fully to keep their arrays in registers (scratch otherwise).
EXTRA_FLAGS = {"hash.hip": ["-mllvm", "-enable-misched=0"], "accumulate.hip": ["-mllvm", "-pragma-unroll-threshold=200000"],
               "tie.hip": ["-mllvm", "-pragma-unroll-threshold=200000"]}       # k_tie_rows batches as k_args_terms does


def _extra(src: str) -> list:
    """Per-file flags; the generated eval_check units share theirs with the load-time compiler (circuits/jit.py)."""
    if src.startswith("eval_check_gen"):
        from .circuits import codegen
        return EXTRA_FLAGS.get(src, []) + codegen.KERNEL_FLAGS
    return EXTRA_FLAGS.get(src, [])


def _deps_digest(src: str) -> str:
    h = hashlib.sha256()
    files = [os.path.join(CSRC, src)]
    files += sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h"))
    files += [os.path.join(ROOT, "include", f) for f in sorted(os.listdir(os.path.join(ROOT, "include")))]
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(FLAGS + _extra(src)).encode())
    return h.hexdigest()


def _compile(src: str, force: bool) -> str:
    obj = os.path.join(OBJ_DIR, src.replace(".hip", ".o"))
    stamp = obj + ".sha"
    digest = _deps_digest(src)
    if not force and os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == digest:
        return obj
    if src.startswith("eval_check_gen"):
        # a generated eval_check unit is compiled only after the exact bound verifier (circuits/bounds.py: it reads the emitted text,
        # shares nothing with the generator) has found no 64-bit sum that can wrap and no reduction outside its domain
        from .circuits import bounds
        with open(os.path.join(CSRC, src)) as fh:
            violations, _ = bounds.check_source(fh.read(), src)
        if violations:
            raise RuntimeError(f"{src}: the generated kernels are NOT within bounds (circuits/codegen.py's lazy-arithmetic accounting is wrong); "
                               f"not compiled:\n" + "\n".join(violations[:5]))
    cmd = [HIPCC, *FLAGS, *_extra(src), "-c", os.path.join(CSRC, src), "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr[-4000:]}")
    with open(stamp, "w") as fh:
        fh.write(digest)
    return obj


def generate_eval_check() -> list:
    """Emit csrc/eval_check_gen*.hip: straight-line eval_check kernels for the shipped circuits (one translation unit per
    part of a split constraint system, so that the parts compile in parallel).  Returns the generated file names."""
    from .circuits import codegen
    return codegen.write_generated(CSRC)


def generate_circuit_descs() -> str:
    """Emit csrc/circuit_descs_gen.hip: the shipped circuit DESCRIPTIONS as data inside the library (zkh_shipped_circuit_desc), so
    that a host without Python has the circuits — SYN-*, KECCAK-F, P2-JOIN and the RECURSION circuit its joins verify — and can
    build the recursion programs itself (zkh_rec_build_program).  Upstream compiles its circuits into the prover the same way."""
    import numpy as np
    from .circuits import codegen
    lines = ["// GENERATED by zeth_amd/build.py generate_circuit_descs — do not edit.  The shipped circuit descriptions (circuits/*.py) as data.",
             "#include <cstddef>", "#include <cstdint>", '#include "common.h"', ""]
    names = []
    for name, desc in codegen.shipped().items():
        d = np.asarray(desc, dtype=np.uint32)
        names.append((name, d.size))
        lines.append(f"static const uint32_t desc_{name}[{d.size}] = {{")
        for i in range(0, d.size, 16):
            lines.append("    " + ", ".join(f"0x{int(w):x}" for w in d[i:i + 16]) + ",")
        lines.append("};")
    lines += ["", "namespace {", "struct Shipped { const char* name; const uint32_t* words; size_t n; };", "const Shipped k_shipped[] = {"]
    lines += [f'    {{"{n}", desc_{n}, {sz}}},' for n, sz in names]
    lines += ["};", "}  // namespace", "",
              'extern "C" size_t zkh_shipped_circuit_count() { return sizeof(k_shipped) / sizeof(k_shipped[0]); }',
              'extern "C" const char* zkh_shipped_circuit_name(size_t i) { return i < zkh_shipped_circuit_count() ? k_shipped[i].name : nullptr; }',
              'extern "C" const char* zkh_shipped_circuit_desc(const char* name, const uint32_t** words, size_t* n_words) {',
              '    ZKH_REQUIRE(name && words && n_words, "shipped_circuit_desc: null argument");',
              "    for (const Shipped& s : k_shipped)",
              "        if (strcmp(s.name, name) == 0) { *words = s.words; *n_words = s.n; return nullptr; }",
              '    return zkh::make_err("shipped_circuit_desc: no circuit named %s is built into this library", name);',
              "}", ""]
    src = "\n".join(lines)
    path = os.path.join(CSRC, "circuit_descs_gen.hip")
    try:
        with open(path) as fh:
            if fh.read() == src:
                return "circuit_descs_gen.hip"
    except FileNotFoundError:
        pass
    with open(path, "w") as fh:
        fh.write(src)
    return "circuit_descs_gen.hip"


def build_examples() -> str:
    """examples/seal_segments (the session written out against the low-level entry points) and examples/prove_session (the
    same session as one zkh_session_prove call): plain g++ consumers of include/zkhal.h (no HIP headers, no Python).
    Returns the path of seal_segments."""
    outs = []
    for name in ("seal_segments", "prove_session", "verify_receipts"):
        src = os.path.join(ROOT, "examples", name + ".cpp")
        out = os.path.join(ROOT, "examples", name)
        outs.append(out)
        deps = [src, os.path.join(ROOT, "include", "zkhal.h"), LIB]
        if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
            continue
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", out, "-L", HERE,
               "-lzkhal_mi355x", "-Wl,-rpath,$ORIGIN/../zeth_amd", "-Wl,-rpath-link,/opt/rocm/lib", "-lpthread"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"g++ failed for examples/{name}.cpp:\n{r.stderr[-4000:]}")
    return outs[0]


def build_oracle() -> None:
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


def build(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(OBJ_DIR, exist_ok=True)
    sources = SOURCES + generate_eval_check() + [generate_circuit_descs()]
    wanted = {s.replace(".hip", ".o") for s in sources}
    for f in os.listdir(OBJ_DIR):                       # objects of generated units that no longer exist
        if f.startswith("eval_check_gen") and f.endswith(".o") and f not in wanted:
            os.remove(os.path.join(OBJ_DIR, f))
    with ThreadPoolExecutor(max_workers=min(os.cpu_count() or 4, len(sources))) as ex:
        objs = list(ex.map(lambda s: _compile(s, force), sources))
    newest = max(os.path.getmtime(o) for o in objs)
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr[-4000:]}")
    if not VARIANT:
        build_examples()
    if verbose:
        print("built", LIB)
    return LIB


def ensure_built(oracle: bool = False, verbose: bool = False) -> str:
    """Build the library (and optionally the CPU oracle, the checker) unless it is already there and current — what a
    SOURCE-ONLY snapshot needs before anything can run (the GPU box receives no built artefacts: .gpurunignore).  Safe to call
    from several processes at once (the ranks of one bench launch): an exclusive file lock serialises them and every caller but
    the first finds the work done.  The build is incremental (per-object dependency digests), so a current tree costs ~1 s.
    A tree whose recorded digest is current is only read, never written (no lock file): a process of another account, or one
    that may not write the checkout, can use a build it did not make."""
    import fcntl
    stamp = os.path.join(OBJ_DIR, ".tree.sha")
    oracle_built = lambda: any(f.endswith(".so") for f in os.listdir(os.path.join(ROOT, "oracle")))   # (building the checker is not using it)
    try:
        with open(stamp) as fh:
            if os.path.exists(LIB) and fh.read() == _tree_digest() and (not oracle or os.environ.get("ZKH_NO_ORACLE_BUILD") or oracle_built()):
                return LIB
    except OSError:
        pass
    os.makedirs(OBJ_DIR, exist_ok=True)
    with open(os.path.join(OBJ_DIR, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            digest = _tree_digest()
            current = os.path.exists(LIB) and os.path.exists(stamp) and open(stamp).read() == digest
            if not current:
                build(verbose=verbose)
                with open(stamp, "w") as fh:
                    fh.write(digest)
            if oracle and not os.environ.get("ZKH_NO_ORACLE_BUILD") and not (current and oracle_built()):
                build_oracle()
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB


def record_tree() -> None:
    """Record the tree digest of the build just made (build() + build_oracle()), so that ensure_built() finds it current and only
    reads it.  Written whole under a temporary name and renamed: a reader sees the old stamp or the new one, never a part."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    stamp = os.path.join(OBJ_DIR, ".tree.sha")
    with open(stamp + ".tmp", "w") as fh:
        fh.write(_tree_digest())
    os.replace(stamp + ".tmp", stamp)


def _tree_digest() -> str:
    """Everything the library is built from: hand-written csrc/, include/, the circuit generators, the flags."""
    h = hashlib.sha256()
    files = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))
             if (f.endswith(".hip") or f.endswith(".h")) and not f.startswith("eval_check_gen") and f != "circuit_descs_gen.hip"]
    files += [os.path.join(ROOT, "include", f) for f in sorted(os.listdir(os.path.join(ROOT, "include")))]
    files += [os.path.join(HERE, "circuits", f) for f in sorted(os.listdir(os.path.join(HERE, "circuits"))) if f.endswith((".py", ".json"))]
    files += [os.path.abspath(__file__)] + [os.path.join(ROOT, "examples", f) for f in sorted(os.listdir(os.path.join(ROOT, "examples"))) if f.endswith(".cpp")]
    files += [os.path.join(ROOT, "oracle", f) for f in sorted(os.listdir(os.path.join(ROOT, "oracle"))) if f.endswith((".c", ".h")) or f == "Makefile"]
    for f in files:
        with open(f, "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
    build_oracle()
