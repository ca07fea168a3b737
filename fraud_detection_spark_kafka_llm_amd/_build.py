"""In-tree build of the native core (``_C.so``) for gfx950.

Kernels (``csrc/*.hip``) are compiled by ``hipcc --offload-arch=gfx950`` without torch headers
(fast, a few seconds each); host C++ (``csrc/*.cpp``) and the pybind11/torch binding TU are
compiled by ``hipcc`` as host code. Objects are cached by a content hash of the source plus
every header in ``csrc/``, so an unchanged tree rebuilds nothing. The shared object links
against the HIP runtime that torch itself loads (same soname ``libamdhip64.so.7``), so the
extension never brings a second HIP runtime into the process.

Usage: ``python -m fraud_detection_spark_kafka_llm_amd._build [--force] [-j N]``.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import hashlib
import os
import shutil
import subprocess
import sys
import sysconfig
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
REPO = PKG_DIR.parent
CSRC = REPO / "csrc"
BUILD = REPO / "build" / "native"
TARGET = PKG_DIR / "_C.so"
ARCH = os.environ.get("FDX_OFFLOAD_ARCH", "gfx950")


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found (ROCm toolchain required to build the native core)")


def _torch_paths():
    import torch
    import torch.utils.cpp_extension as ce

    inc = [Path(p) for p in ce.include_paths()]
    lib = Path(ce.library_paths()[0])
    abi = int(torch._C._GLIBCXX_USE_CXX11_ABI)
    return inc, lib, abi


def _headers_digest() -> str:
    h = hashlib.sha256()
    for p in sorted(CSRC.glob("*.h")):
        h.update(p.name.encode())
        h.update(p.read_bytes())
    return h.hexdigest()


def _obj_for(src: Path, flags: list[str], hdr: str) -> Path:
    h = hashlib.sha256()
    h.update(src.read_bytes())
    h.update(hdr.encode())
    h.update(" ".join(flags).encode())
    return BUILD / f"{src.stem}.{src.suffix[1:]}.{h.hexdigest()[:16]}.o"


def _run(cmd: list[str]) -> None:
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"native build failed:\n{' '.join(cmd)}\n{res.stdout}\n{res.stderr}")


def build(force: bool = False, jobs: int | None = None, verbose: bool = False) -> Path:
    hipcc = _hipcc()
    inc, lib, abi = _torch_paths()
    BUILD.mkdir(parents=True, exist_ok=True)
    hdr = _headers_digest()
    common = ["-O3", "-fPIC", "-std=c++17", f"-I{CSRC}", "-I/opt/rocm/include", "-Wno-unused-result", "-Wno-deprecated-declarations"]
    # No -ffast-math: reassociation would break the bitwise host/device agreement of the fp64
    # reductions (and Spark parity); kernels opt into fast paths explicitly where it is safe.
    kernel_flags = common + ["-x", "hip", f"--offload-arch={ARCH}", "-ffp-contract=off"]
    # host C++ (CPU path): no GPU code, plain optimisation.
    host_flags = common + ["-x", "c++", "-D__HIP_PLATFORM_AMD__=1", "-march=x86-64-v2", "-pthread",
                           "-ffp-contract=off"]
    py_inc = sysconfig.get_paths()["include"]
    bind_flags = common + ["-x", "c++", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
                           f"-D_GLIBCXX_USE_CXX11_ABI={abi}", "-DTORCH_EXTENSION_NAME=_C",
                           "-DTORCH_API_INCLUDE_EXTENSION_H", f"-I{py_inc}"] + [f"-I{p}" for p in inc]
    jobs_list = []
    for src in sorted(CSRC.glob("*.hip")):
        jobs_list.append((src, kernel_flags))
    for src in sorted(CSRC.glob("*.cpp")):
        jobs_list.append((src, bind_flags if src.name.startswith("bindings") else host_flags))

    objs: list[Path] = []
    todo = []
    for src, fl in jobs_list:
        obj = _obj_for(src, fl, hdr)
        objs.append(obj)
        if force or not obj.exists():
            todo.append((src, fl, obj))

    def compile_one(item):
        src, fl, obj = item
        tmp = obj.with_suffix(".tmp.o")
        cmd = [hipcc, *fl, "-c", str(src), "-o", str(tmp)]
        if verbose:
            print(" ".join(cmd), flush=True)
        _run(cmd)
        tmp.replace(obj)
        return src.name

    if todo:
        n = jobs or min(len(todo), max(1, (os.cpu_count() or 4)))
        with cf.ThreadPoolExecutor(n) as ex:
            for name in ex.map(compile_one, todo):
                if verbose:
                    print(f"[fdx-build] compiled {name}", flush=True)

    link_key = hashlib.sha256("".join(str(o) for o in objs).encode()).hexdigest()[:16]
    stamp = BUILD / "link.stamp"
    if force or not TARGET.exists() or not stamp.exists() or stamp.read_text() != link_key:
        tmp = TARGET.with_suffix(".tmp.so")
        cmd = [hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", *map(str, objs), "-o", str(tmp),
               f"-L{lib}", "-lc10", "-lc10_hip", "-ltorch", "-ltorch_cpu", "-ltorch_hip", "-ltorch_python",
               f"-Wl,-rpath,{lib}", "-pthread"]
        if verbose:
            print(" ".join(cmd), flush=True)
        _run(cmd)
        tmp.replace(TARGET)
        stamp.write_text(link_key)
        # drop stale objects of older source revisions
        keep = {o.name for o in objs}
        for o in BUILD.glob("*.o"):
            if o.name not in keep:
                o.unlink(missing_ok=True)
    return TARGET


# identical private string literals that libstdc++ headers instantiate in several TUs trip ASan's
# ODR check (false positive); every other check stays on, and UBSan findings abort.
SELFTEST_ENV = {"ASAN_OPTIONS": "detect_odr_violation=0:abort_on_error=1:detect_leaks=1",
                "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
HOST_SOURCES = ("text_cpu.cpp", "sparse_cpu.cpp", "tree_cpu.cpp", "json_text.cpp", "json_encode.cpp")


def build_host_selftest(sanitize: bool = True, out: Path | None = None) -> Path:
    """Debug target of SURVEY §5.2: the host (CPU) implementations + ``csrc/tests/host_selftest.cpp``
    as a standalone executable, built with AddressSanitizer + UndefinedBehaviorSanitizer (host
    code only: no device code is compiled into it)."""
    hipcc = _hipcc()
    out = out or (BUILD / ("host_selftest_asan" if sanitize else "host_selftest"))
    out.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O1", "-g", "-std=c++17", f"-I{CSRC}", "-I/opt/rocm/include", "-x", "c++", "-D__HIP_PLATFORM_AMD__=1",
             "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize",
                  ]
    # one translation unit (unity build): inline functions of libstdc++ then exist once, so ASan
    # does not see the same COMDAT string literal registered by several objects (false ODR report)
    unity = out.parent / "host_selftest_unity.cpp"
    unity.write_text("".join(f'#include "{CSRC / s}"\n' for s in HOST_SOURCES)
                     + f'#include "{CSRC / "tests" / "host_selftest.cpp"}"\n')
    link = ["-fsanitize=address,undefined"] if sanitize else []
    _run([hipcc, *flags, str(unity), "-o", str(out), "-pthread", *link])
    return out


def build_contrib_selftest(sanitize: bool = True, out: Path | None = None) -> Path:
    """``csrc/tests/contrib_selftest.cpp`` + the TreeSHAP host twin (``contrib_cpu.cpp``) as a
    standalone executable under AddressSanitizer + UndefinedBehaviorSanitizer, built like
    ``build_host_selftest`` (host code only, one translation unit)."""
    hipcc = _hipcc()
    out = out or (BUILD / ("contrib_selftest_asan" if sanitize else "contrib_selftest"))
    out.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O1", "-g", "-std=c++17", f"-I{CSRC}", "-I/opt/rocm/include", "-x", "c++", "-D__HIP_PLATFORM_AMD__=1",
             "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize"]
    unity = out.parent / "contrib_selftest_unity.cpp"
    unity.write_text(f'#include "{CSRC / "contrib_cpu.cpp"}"\n#include "{CSRC / "tests" / "contrib_selftest.cpp"}"\n')
    link = ["-fsanitize=address,undefined"] if sanitize else []
    _run([hipcc, *flags, str(unity), "-o", str(out), "-pthread", *link])
    return out


def build_eval_selftest(sanitize: bool = True, out: Path | None = None) -> Path:
    """``csrc/tests/eval_selftest.cpp`` + the validation-monitoring host twins (``eval_cpu.cpp``) as a
    standalone executable under AddressSanitizer + UndefinedBehaviorSanitizer, built like
    ``build_contrib_selftest`` (host code only, one translation unit)."""
    hipcc = _hipcc()
    out = out or (BUILD / ("eval_selftest_asan" if sanitize else "eval_selftest"))
    out.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O1", "-g", "-std=c++17", f"-I{CSRC}", "-I/opt/rocm/include", "-x", "c++", "-D__HIP_PLATFORM_AMD__=1",
             "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize"]
    unity = out.parent / "eval_selftest_unity.cpp"
    unity.write_text(f'#include "{CSRC / "eval_cpu.cpp"}"\n#include "{CSRC / "tests" / "eval_selftest.cpp"}"\n')
    link = ["-fsanitize=address,undefined"] if sanitize else []
    _run([hipcc, *flags, str(unity), "-o", str(out), "-pthread", *link])
    return out


def build_ngram_selftest(sanitize: bool = True, out: Path | None = None) -> Path:
    """``csrc/tests/ngram_selftest.cpp`` + the fused featurizer's host twin (``text_cpu.cpp``) as a
    standalone executable under AddressSanitizer + UndefinedBehaviorSanitizer, built like
    ``build_eval_selftest`` (host code only, one translation unit)."""
    hipcc = _hipcc()
    out = out or (BUILD / ("ngram_selftest_asan" if sanitize else "ngram_selftest"))
    out.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O1", "-g", "-std=c++17", f"-I{CSRC}", "-I/opt/rocm/include", "-x", "c++", "-D__HIP_PLATFORM_AMD__=1",
             "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize"]
    unity = out.parent / "ngram_selftest_unity.cpp"
    unity.write_text(f'#include "{CSRC / "text_cpu.cpp"}"\n#include "{CSRC / "tests" / "ngram_selftest.cpp"}"\n')
    link = ["-fsanitize=address,undefined"] if sanitize else []
    _run([hipcc, *flags, str(unity), "-o", str(out), "-pthread", *link])
    return out


def build_cls_selftest(sanitize: bool = True, out: Path | None = None) -> Path:
    """``csrc/tests/cls_selftest.cpp`` + the fused featurizer's host twin (``text_cpu.cpp``) as a
    standalone executable under AddressSanitizer + UndefinedBehaviorSanitizer, built like
    ``build_ngram_selftest`` (host code only, one translation unit): the class-score tail."""
    hipcc = _hipcc()
    out = out or (BUILD / ("cls_selftest_asan" if sanitize else "cls_selftest"))
    out.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O1", "-g", "-std=c++17", f"-I{CSRC}", "-I/opt/rocm/include", "-x", "c++", "-D__HIP_PLATFORM_AMD__=1",
             "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize"]
    unity = out.parent / "cls_selftest_unity.cpp"
    unity.write_text(f'#include "{CSRC / "text_cpu.cpp"}"\n#include "{CSRC / "tests" / "cls_selftest.cpp"}"\n')
    link = ["-fsanitize=address,undefined"] if sanitize else []
    _run([hipcc, *flags, str(unity), "-o", str(out), "-pthread", *link])
    return out


def build_lr_selftest(sanitize: bool = True, out: Path | None = None) -> Path:
    """``csrc/tests/lr_selftest.cpp`` + the elastic-net logistic-regression host twins (``lr_cpu.cpp``, and
    ``sparse_cpu.cpp`` for the SpMV the margins must equal) as a standalone executable under
    AddressSanitizer + UndefinedBehaviorSanitizer, built like ``build_eval_selftest`` (host code only,
    one translation unit)."""
    hipcc = _hipcc()
    out = out or (BUILD / ("lr_selftest_asan" if sanitize else "lr_selftest"))
    out.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O1", "-g", "-std=c++17", f"-I{CSRC}", "-I/opt/rocm/include", "-x", "c++", "-D__HIP_PLATFORM_AMD__=1",
             "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize"]
    unity = out.parent / "lr_selftest_unity.cpp"
    unity.write_text("".join(f'#include "{CSRC / s}"\n' for s in ("sparse_cpu.cpp", "lr_cpu.cpp"))
                     + f'#include "{CSRC / "tests" / "lr_selftest.cpp"}"\n')
    link = ["-fsanitize=address,undefined"] if sanitize else []
    _run([hipcc, *flags, str(unity), "-o", str(out), "-pthread", *link])
    return out


def build_sim_selftest(sanitize: bool = True, out: Path | None = None) -> Path:
    """``csrc/tests/sim_selftest.cpp`` + the top-k cosine retrieval host twins (``sim_cpu.cpp``) as a
    standalone executable under AddressSanitizer + UndefinedBehaviorSanitizer, built like
    ``build_lr_selftest`` (host code only, one translation unit)."""
    hipcc = _hipcc()
    out = out or (BUILD / ("sim_selftest_asan" if sanitize else "sim_selftest"))
    out.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O1", "-g", "-std=c++17", f"-I{CSRC}", "-I/opt/rocm/include", "-x", "c++", "-D__HIP_PLATFORM_AMD__=1",
             "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize"]
    unity = out.parent / "sim_selftest_unity.cpp"
    unity.write_text(f'#include "{CSRC / "sim_cpu.cpp"}"\n#include "{CSRC / "tests" / "sim_selftest.cpp"}"\n')
    link = ["-fsanitize=address,undefined"] if sanitize else []
    _run([hipcc, *flags, str(unity), "-o", str(out), "-pthread", *link])
    return out


def build_nb_selftest(sanitize: bool = True, out: Path | None = None) -> Path:
    """``csrc/tests/nb_selftest.cpp`` + the Naive Bayes host twins (``nb_cpu.cpp``) as a standalone
    executable under AddressSanitizer + UndefinedBehaviorSanitizer, built like ``build_sim_selftest``
    (host code only, one translation unit)."""
    hipcc = _hipcc()
    out = out or (BUILD / ("nb_selftest_asan" if sanitize else "nb_selftest"))
    out.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O1", "-g", "-std=c++17", f"-I{CSRC}", "-I/opt/rocm/include", "-x", "c++", "-D__HIP_PLATFORM_AMD__=1",
             "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize"]
    unity = out.parent / "nb_selftest_unity.cpp"
    unity.write_text(f'#include "{CSRC / "nb_cpu.cpp"}"\n#include "{CSRC / "tests" / "nb_selftest.cpp"}"\n')
    link = ["-fsanitize=address,undefined"] if sanitize else []
    _run([hipcc, *flags, str(unity), "-o", str(out), "-pthread", *link])
    return out


def build_mlr_selftest(sanitize: bool = True, out: Path | None = None) -> Path:
    """``csrc/tests/mlr_selftest.cpp`` + the multinomial logistic-regression host twin (``mlr_cpu.cpp``, and
    ``nb_cpu.cpp`` for the class scores the margins must equal) as a standalone executable under
    AddressSanitizer + UndefinedBehaviorSanitizer, built like ``build_nb_selftest`` (host code only,
    one translation unit)."""
    hipcc = _hipcc()
    out = out or (BUILD / ("mlr_selftest_asan" if sanitize else "mlr_selftest"))
    out.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O1", "-g", "-std=c++17", f"-I{CSRC}", "-I/opt/rocm/include", "-x", "c++", "-D__HIP_PLATFORM_AMD__=1",
             "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize"]
    unity = out.parent / "mlr_selftest_unity.cpp"
    unity.write_text("".join(f'#include "{CSRC / s}"\n' for s in ("nb_cpu.cpp", "mlr_cpu.cpp"))
                     + f'#include "{CSRC / "tests" / "mlr_selftest.cpp"}"\n')
    link = ["-fsanitize=address,undefined"] if sanitize else []
    _run([hipcc, *flags, str(unity), "-o", str(out), "-pthread", *link])
    return out


def build_softprob_selftest(sanitize: bool = True, out: Path | None = None) -> Path:
    """``csrc/tests/softprob_selftest.cpp`` + the multi-class boosting host twins (``softprob_cpu.cpp``) as a
    standalone executable under AddressSanitizer + UndefinedBehaviorSanitizer, built like
    ``build_mlr_selftest`` (host code only, one translation unit)."""
    hipcc = _hipcc()
    out = out or (BUILD / ("softprob_selftest_asan" if sanitize else "softprob_selftest"))
    out.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O1", "-g", "-std=c++17", f"-I{CSRC}", "-I/opt/rocm/include", "-x", "c++", "-D__HIP_PLATFORM_AMD__=1",
             "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize"]
    unity = out.parent / "softprob_selftest_unity.cpp"
    unity.write_text(f'#include "{CSRC / "softprob_cpu.cpp"}"\n#include "{CSRC / "tests" / "softprob_selftest.cpp"}"\n')
    link = ["-fsanitize=address,undefined"] if sanitize else []
    _run([hipcc, *flags, str(unity), "-o", str(out), "-pthread", *link])
    return out


def build_svc_selftest(sanitize: bool = True, out: Path | None = None) -> Path:
    """``csrc/tests/svc_selftest.cpp`` + the linear SVC host twin (``svc_cpu.cpp``) as a standalone
    executable under AddressSanitizer + UndefinedBehaviorSanitizer, built like ``build_mlr_selftest``
    (host code only, one translation unit)."""
    hipcc = _hipcc()
    out = out or (BUILD / ("svc_selftest_asan" if sanitize else "svc_selftest"))
    out.parent.mkdir(parents=True, exist_ok=True)
    flags = ["-O1", "-g", "-std=c++17", f"-I{CSRC}", "-I/opt/rocm/include", "-x", "c++", "-D__HIP_PLATFORM_AMD__=1",
             "-pthread", "-ffp-contract=off", "-fno-omit-frame-pointer"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-gpu-sanitize"]
    unity = out.parent / "svc_selftest_unity.cpp"
    unity.write_text(f'#include "{CSRC / "svc_cpu.cpp"}"\n#include "{CSRC / "tests" / "svc_selftest.cpp"}"\n')
    link = ["-fsanitize=address,undefined"] if sanitize else []
    _run([hipcc, *flags, str(unity), "-o", str(out), "-pthread", *link])
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--force", action="store_true")
    ap.add_argument("-j", "--jobs", type=int, default=None)
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("--host-selftest", action="store_true", help="build + run the ASan/UBSan host self-test")
    ap.add_argument("--contrib-selftest", action="store_true",
                    help="build + run the ASan/UBSan self-test of the TreeSHAP host twin")
    ap.add_argument("--eval-selftest", action="store_true",
                    help="build + run the ASan/UBSan self-test of the validation-monitoring host twins")
    ap.add_argument("--ngram-selftest", action="store_true",
                    help="build + run the ASan/UBSan self-test of the n-gram mode of the featurizer's host twin")
    ap.add_argument("--lr-selftest", action="store_true",
                    help="build + run the ASan/UBSan self-test of the elastic-net logistic-regression host twins")
    ap.add_argument("--sim-selftest", action="store_true",
                    help="build + run the ASan/UBSan self-test of the top-k cosine retrieval host twins")
    ap.add_argument("--nb-selftest", action="store_true",
                    help="build + run the ASan/UBSan self-test of the Naive Bayes host twins")
    ap.add_argument("--mlr-selftest", action="store_true",
                    help="build + run the ASan/UBSan self-test of the multinomial logistic-regression host twin")
    ap.add_argument("--cls-selftest", action="store_true",
                    help="build + run the ASan/UBSan self-test of the class-score tail of the featurizer's host twin")
    ap.add_argument("--softprob-selftest", action="store_true",
                    help="build + run the ASan/UBSan self-test of the multi-class boosting host twins")
    ap.add_argument("--svc-selftest", action="store_true",
                    help="build + run the ASan/UBSan self-test of the linear SVC host twin")
    args = ap.parse_args(argv)
    if args.svc_selftest:
        return subprocess.run([str(build_svc_selftest())], env={**os.environ, **SELFTEST_ENV}).returncode
    if args.softprob_selftest:
        return subprocess.run([str(build_softprob_selftest())], env={**os.environ, **SELFTEST_ENV}).returncode
    if args.cls_selftest:
        return subprocess.run([str(build_cls_selftest())], env={**os.environ, **SELFTEST_ENV}).returncode
    if args.mlr_selftest:
        return subprocess.run([str(build_mlr_selftest())], env={**os.environ, **SELFTEST_ENV}).returncode
    if args.nb_selftest:
        return subprocess.run([str(build_nb_selftest())], env={**os.environ, **SELFTEST_ENV}).returncode
    if args.sim_selftest:
        return subprocess.run([str(build_sim_selftest())], env={**os.environ, **SELFTEST_ENV}).returncode
    if args.lr_selftest:
        return subprocess.run([str(build_lr_selftest())], env={**os.environ, **SELFTEST_ENV}).returncode
    if args.ngram_selftest:
        return subprocess.run([str(build_ngram_selftest())], env={**os.environ, **SELFTEST_ENV}).returncode
    if args.host_selftest or args.contrib_selftest or args.eval_selftest:
        exe = build_host_selftest() if args.host_selftest else \
            (build_contrib_selftest() if args.contrib_selftest else build_eval_selftest())
        return subprocess.run([str(exe)], env={**os.environ, **SELFTEST_ENV}).returncode
    path = build(force=args.force, jobs=args.jobs, verbose=args.verbose)
    print(f"built {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
