"""The build driver of libpcc_hip.so and the checks it runs on the generated code: ``build()`` (``make -C csrc``; hipcc
--offload-arch=gfx950), the compiler's per-kernel resource remarks, and the LDS-read lint of conv_small_kernel."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libpcc_hip.so")

# resources file stem (build/<stem>.resources.txt) -> substrings of the names of the kernels that must run out of registers alone
NO_SCRATCH = {
    # the MFMA convolutions (a spilled accumulator is a 20x slowdown, and conv_small_kernel's inline-assembly LDS reads sit
    # behind a hand-placed s_waitcnt that the compiler does not see: a spilled or copied operand register would be read before
    # its data has landed, silently)
    "conv": ("conv_small_kernel", "conv_mfma_buf_kernel", "conv_mfma_kernel"),
    # the lane-parallel range coder (csrc/rans_lanes.hip): one thread carries one serial state chain, and a spilled state or
    # batch register would put a scratch round trip into every link of it
    "rans_lanes": ("rans_lanes_encode_kernel", "rans_lanes_pack_kernel", "rans_lanes_decode_kernel"),
    # the channelwise window convolution (csrc/chconv.hip): up to 1,331 probes and adds per output element run out of one
    # accumulator and a handful of probe registers, and a spill would sit inside that loop
    "chconv": ("chconv_kernel",),
    # the training augmentation (csrc/augment.hip): the jitter's chain of four operations in a per-item order is unrolled over
    # registers, and an indexed (scratch) copy of it would sit in every point's path; the rotation's first-row set
    # (csrc/first_rows.h: one entry covers every instantiation, the names are matched as substrings of the mangled ones)
    "augment": ("jitter_partial_kernel", "jitter_mean_kernel", "jitter_apply_kernel", "first_rows_clear_kernel",
                "first_rows_insert_kernel", "first_rows_flag_kernel", "first_rows_finalize_kernel"),
    # the surface normals (csrc/normals.hip): the 3 x 3 Jacobi iteration runs over named scalars, and an indexed (scratch) copy
    # of the matrix would put a memory round trip into every one of its 36 rotations
    "normals": ("estimate_normals_kernel",),
    # the voxelisation (csrc/voxelize.hip): the channel loops run over a run-time count out of a handful of registers; an indexed
    # (scratch) copy of a point's channels would sit in front of every atomic of the accumulation pass
    "voxelize": ("first_rows_clear_kernel", "first_rows_insert_kernel", "first_rows_flag_kernel", "first_rows_finalize_kernel",
                 "voxelize_accumulate_kernel"),
    # the position scaling (csrc/rescale.hip): the cell set is the voxelisation's, and the lattice walk keeps a point, its cell and
    # the running best in registers through up to 27 table probes per shell; a spill would sit inside that loop
    "rescale": ("first_rows_insert_kernel", "first_rows_finalize_kernel", "scaled_accumulate_kernel", "scaled_transfer_kernel"),
    # RAHT (csrc/raht.hip): a step is two gathered float64 rows in, two out; a spill would sit between the gather and the store
    "raht": ("raht_plan_kernel", "raht_step_kernel", "raht_fold_kernel"),
    # the perceptual metric (csrc/pcqm.hip): 20 running sums per point live through up to 4,218 probes and gathers; a spilled
    # one would put a scratch round trip behind every neighbour.  The kappa kernel shares the normals' Jacobi over named scalars
    "pcqm": ("surface_variation_kernel", "pcqm_features_kernel"),
    # the views (csrc/render.hip; the two templates, so both instantiations of each, orthographic and camera): three emulated
    # 64-bit divisions per point of a camera view sit in front of up to 256 atomics or reads; a spill among their operands would
    # be a scratch round trip per point in two kernels that otherwise touch only the z-buffer
    "render": ("splat_kernel", "gather_kernel"),
}


def build(force=False):
    """Compile libpcc_hip.so for gfx950 (cross-compiles without a GPU)."""
    args = ["make", "-s", "-C", os.path.join(_HERE, "csrc"), "-j4"]
    if force:
        subprocess.check_call(args + ["clean"])
    subprocess.check_call(args)
    for stem, kernels in NO_SCRATCH.items():
        check_kernel_resources(os.path.join(_HERE, "build", stem + ".resources.txt"), kernels)
    check_small_kernel_lds_reads()
    return SO_PATH


def check_small_kernel_lds_reads(obj=None):
    """conv_small_kernel reads its MFMA operands with inline-assembly ds_read_b128, which the compiler does not count in
    lgkmcnt; the kernel waits for them with a hand-placed s_waitcnt (csrc/conv.hip, pick()).  That is correct only while no
    instruction touches a destination register of such a read between the read and the wait — a register copy or spill the
    compiler inserted there would move stale data, silently.  This lints the generated code: the device code object
    is extracted from build/conv.o, disassembled, and every conv_small_kernel instantiation is walked; any mention of a pending
    read's registers before the next `s_waitcnt lgkmcnt(0)` fails the build.  -> number of reads checked."""
    import glob
    import shutil
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    obj = obj or os.path.join(_HERE, "build", "conv.o")
    if not os.path.exists(objdump) or not os.path.exists(obj):
        raise RuntimeError(f"cannot lint conv_small_kernel: {objdump} or {obj} is missing")
    tmp = os.path.join(_HERE, "build", "_lint")
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(tmp)
    local = os.path.join(tmp, "conv.o")
    shutil.copy(obj, local)
    subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=tmp)
    cos = [f for f in glob.glob(local + ".*") if "amdgcn" in f]
    if not cos:
        raise RuntimeError("cannot lint conv_small_kernel: no device code object in build/conv.o")
    dis = subprocess.run([objdump, "-d", cos[0]], check=True, capture_output=True, text=True).stdout
    shutil.rmtree(tmp, ignore_errors=True)
    return lint_lds_reads(dis)


def lint_lds_reads(dis, kernel="conv_small_kernel"):
    """the walk of check_small_kernel_lds_reads over a disassembly listing (llvm-objdump -d): -> reads checked, or RuntimeError"""
    import re

    def regs(operand):
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
        if m:
            return set(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.fullmatch(r"v(\d+)", operand)
        return {int(m.group(1))} if m else set()

    checked, func, pending = 0, None, {}
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            func = m.group(1) if kernel in m.group(1) else None
            pending = {}
            continue
        if func is None:
            continue
        text = line.split("//")[0].strip()
        if not text:
            continue
        parts = text.split(None, 1)
        mnem = parts[0]
        ops = [o.strip().split(" ")[0] for o in parts[1].split(",")] if len(parts) > 1 else []
        if mnem == "s_waitcnt" and "lgkmcnt(0)" in text:
            pending = {}
            continue
        touched = set()
        for o in ops:
            touched |= regs(o)
        clash = touched & set(pending)
        if mnem == "ds_read_b128":
            dest = regs(ops[0])
            clash = (touched - dest) & set(pending) | (dest & set(pending))
            if not clash:
                for r_ in dest:
                    pending[r_] = text
                checked += 1
        if clash:
            raise RuntimeError(f"{func}: `{text}` touches v{sorted(clash)} while an LDS read into them is still in flight "
                               f"(`{pending[sorted(clash)[0]]}`): the hand-placed s_waitcnt of conv_small_kernel no longer covers it")
    if not checked:
        raise RuntimeError(f"cannot lint {kernel}: no ds_read_b128 found in its disassembly")
    return checked


def check_kernel_resources(path=None, kernels=None):
    """Parse the compiler's per-kernel resource remarks (csrc/Makefile writes them beside the objects) and fail loudly
    when one of ``kernels`` (default: the convolution kernels, NO_SCRATCH["conv"]) uses scratch memory or spills registers.
    -> {mangled kernel name: (vgprs, scratch)}"""
    import re
    kernels = kernels or NO_SCRATCH["conv"]
    path = path or os.path.join(_HERE, "build", "conv.resources.txt")
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: the library was not built by csrc/Makefile")
    seen, name = {}, None
    vals = {}
    with open(path) as f:
        for line in f:
            m = re.search(r"remark:\s+Function Name: (\S+)", line)
            if m:
                name, vals = m.group(1), {}
                seen[name] = vals
                continue
            m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\d+)", line)
            if m and name:
                vals[m.group(1)] = int(m.group(2))
    bad = {k: v for k, v in seen.items() if any(t in k for t in kernels)
           and (v.get("ScratchSize [bytes/lane]", 0) or v.get("SGPRs Spill", 0) or v.get("VGPRs Spill", 0))}
    checked = [k for k in seen if any(t in k for t in kernels)]
    unmatched = [t for t in kernels if not any(t in k for k in seen)]
    if unmatched:
        raise RuntimeError(f"{path}: no resource remarks for {unmatched} (kernel renamed, or compiler flag dropped?)")
    if bad:
        raise RuntimeError(f"kernels with scratch memory or spills (must be none): {bad}")
    return {k: (seen[k].get("VGPRs"), seen[k].get("ScratchSize [bytes/lane]")) for k in checked}
