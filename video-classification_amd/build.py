"""Build libsfk.so (the C-ABI kernel library of include/sfk.h) with hipcc for gfx950, in-tree."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsfk.so")
SOURCES = ["conv_igemm.hip", "conv_igemm_p8.hip", "conv_halo.hip", "conv_pw.hip", "conv_wgrad.hip", "conv_wgrad_p8.hip", "conv_wgrad_band.hip", "stem_conv.hip", "bn.hip", "bn_tail.hip", "pool_head.hip",
           "optim_misc.hip", "eval_input.hip", "stem2d.hip", "roi_resize.hip", "sgd.hip", "color_jitter.hip", "u8_pool_gather.hip", "pad_resize.hip", "optim_sched.hip", "optim_groups.hip", "clip_mix.hip", "loss_mix.hip", "ema.hip", "u8_pool_warp.hip", "roi_warp.hip"]


def _newer(a, b):
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def build(force: bool = False, verbose: bool = False) -> str:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    deps = [os.path.join(CSRC, "sfk_common.h"), os.path.join(CSRC, "conv_igemm_epi.h"), os.path.join(CSRC, "conv_wgrad_common.h"), os.path.join(CSRC, "conv_wgrad_band_acc.inc"), os.path.join(ROOT, "include", "sfk.h"),
            os.path.join(ROOT, "include", "sfk_stem2d.h"), os.path.join(ROOT, "include", "sfk_u8stem.h"),
            os.path.join(ROOT, "include", "sfk_v2.h"), os.path.join(ROOT, "include", "sfk_aug.h"),
            os.path.join(ROOT, "include", "sfk_pool.h"), os.path.join(ROOT, "include", "sfk_resize.h"),
            os.path.join(ROOT, "include", "sfk_resident.h"), os.path.join(ROOT, "include", "sfk_roi_pool.h"),
            os.path.join(ROOT, "include", "sfk_roi_ragged.h"), os.path.join(ROOT, "include", "sfk_u8stem_pool.h"),
            os.path.join(ROOT, "include", "sfk_optim.h"), os.path.join(ROOT, "include", "sfk_groups.h"),
            os.path.join(ROOT, "include", "sfk_mix.h"), os.path.join(ROOT, "include", "sfk_ema.h"),
            os.path.join(ROOT, "include", "sfk_warp.h"), os.path.join(ROOT, "include", "sfk_roi_warp.h"),
            os.path.join(CSRC, "roi_common.h"), os.path.join(CSRC, "optim_elem.h"), os.path.join(CSRC, "stem_src.h")]
    flags = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    flags += os.environ.get("SFK_EXTRA_FLAGS", "").split()          # experiment builds (tools/), with SFK_LIB_OUT

    def compile_one(src):
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        if force or _newer(s, o) or any(_newer(d, o) for d in deps):
            cmd = [hipcc] + flags + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
            return o, True
        return o, False

    with ThreadPoolExecutor(max_workers=min(4, len(SOURCES))) as ex:
        res = list(ex.map(compile_one, SOURCES))
    objs = [o for o, _ in res]
    if force or any(ch for _, ch in res) or not os.path.exists(LIB):
        subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs, check=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in os.sys.argv, verbose=True))
