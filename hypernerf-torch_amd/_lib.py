"""ctypes binding of the C-ABI shared library (include/hn_kernels.h).

The product path has NO CPU fallback: if the library is missing, or a tensor is not on a
ROCm device, the ops raise.  `load()` is lazy so that module construction, state_dict
handling and program building work on a machine without a GPU (tests -m "not gpu").
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
PRODUCT_LIB_PATH = os.path.join(CSRC, "libhn_hip.so")
# HN_LIB_PATH: run under ANOTHER build of the library (the A/B tools compare prebuilt variants without ever overwriting
# the product library); build() / needs_build() only ever write the product path
LIB_PATH = os.environ.get("HN_LIB_PATH") or PRODUCT_LIB_PATH
SOURCES = ["hn_mlp.hip", "hn_render.hip", "hn_data.hip", "hn_calib.hip", "hn_optim.hip", "hn_metrics.hip", "hn_msssim.hip",
           "hn_geometry.hip", "hn_regularizers.hip", "hn_gif.hip", "hn_simplify.hip", "hn_mesh_render.hip", "hn_fusion.hip",
           "hn_mesh_distance.hip", "hn_lpips.hip", "hn_registration.hip", "hn_texture.hip", "hn_occupancy.hip"]
CSRC_HEADERS = ["hn_common.h", "hn_pack.h", "hn_camera.h", "hn_window.h", "hn_wave.h", "hn_mlp_fwd_body.h", "hn_mlp_bwd_body.h"]
HEADER = os.path.join(os.path.dirname(_HERE), "include", "hn_kernels.h")
BUILD_MACROS = ("HN_REDUCE_SPLIT", "HN_BF16_WAVES", "HN_PROF", "HN_CHUNK_UNITS", "HN_WGRAD_AUX", "HN_WGRAD_STAGES", "HN_WGRAD_MAXSLOT", "HN_BWD_PIPE")     # build-time tuning knobs (A/B experiments)


class HnError(RuntimeError):
    pass


BUILD_CONFIG_KEYS = ("WGRAD_STAGES", "WGRAD_MAXSLOT", "WGRAD_BIAS_MFMA", "CHUNK_UNITS", "WGRAD_BLOCK", "WSTREAM_ASYM",
                     "BF16_WAVES", "WGRAD_AUX")


def _read_build_config(path: str):
    """The build-time knobs of the library at `path`, or None when there is no library (or one older than ABI 340).
    Read from the marker string the library carries (`hn_build_config_text`) WITHOUT dlopen-ing it: this runs at import
    time, and a library that was dlopen-ed once stays mapped under its path — a rebuild that follows (build(force=True))
    would then never be seen by load().  load() cross-checks the text against hn_build_config() of the mapped code."""
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError:
        return None
    m = re.search(rb"HN_BUILD_CONFIG:([0-9, ]+);", blob)
    if m is None:
        return None
    vals = [int(x) for x in m.group(1).decode().replace(" ", "").split(",")]
    return {k: v for k, v in zip(BUILD_CONFIG_KEYS, vals)}


# hn_wgrad_kernel's LDS ring and the weight-stream chunk of the build: host-side mirrors of build-time
# macros in csrc/hn_mlp.hip.  They come from the LIBRARY (hn_build_config) whenever one exists — a library prebuilt
# with other knobs carries its own values; the environment variables (which also drive build()) only stand in before the
# first build, and load() refuses a library that disagrees with the mirrors in use.
BUILD_CONFIG = _read_build_config(LIB_PATH)
_cfg = BUILD_CONFIG or {}
WGRAD_STAGES = _cfg.get("WGRAD_STAGES", int(os.environ.get("HN_WGRAD_STAGES") or 2))
WGRAD_MAXSLOT = _cfg.get("WGRAD_MAXSLOT", int(os.environ.get("HN_WGRAD_MAXSLOT") or 8))
WGRAD_MAX_STAGE_KB = min(8 * WGRAD_MAXSLOT, 160 // WGRAD_STAGES)

_SCALARS = {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64, "long long": C.c_longlong}


def parse_prototypes(text: str) -> dict:
    """{entry point: argtypes}, in declaration order, of every `int hn_*(...);` prototype in `text`.  Not a C parser: it
    knows the parameter shapes include/hn_kernels.h uses (pointers and hnStream_t -> c_void_p, the four scalar kinds, a
    `(void)` list) and raises on anything else instead of guessing."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for start in re.finditer(r"^int (hn_\w+)\(", text, flags=re.M):
        name, rest = start.group(1), re.compile(r"([^()]*)\);").match(text, start.end())
        if rest is None:
            raise HnError(f"{name}: the prototype is not a plain parameter list closed by ');'")
        params = rest.group(1)
        out[name] = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            ctype = " ".join(param.split()[:-1])          # drop the parameter's name
            if "*" in param or ctype == "hnStream_t":
                out[name].append(C.c_void_p)
            elif ctype in _SCALARS:
                out[name].append(_SCALARS[ctype])
            else:
                raise HnError(f"{name}: parameter '{' '.join(param.split())}' has a type the binding does not know")
    return out


_FIELD_SCALARS = {"int8_t": C.c_int8, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64,
                  "uint64_t": C.c_uint64, "float": C.c_float}
_ABI_ITEM = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(HN_\w+)[ \t]*(.*?)[ \t]*$"
                       r"|\btypedef\s+(\w+)\s*\w*\s*\{((?:[^{}]|\{[^{}]*\})*)\}\s*(\w+)\s*;", flags=re.M)


def parse_abi(text: str):
    """(constants, structs) of `text`, each a dict in header order: every `#define HN_NAME <integer literal>` (the
    include guard is skipped) and every `typedef struct [Tag] { ... } Name;` as a ctypes.Structure.  Not a C parser: it
    knows the member shapes include/hn_kernels.h uses (the six fixed-width scalars, any pointer -> c_void_p, an earlier
    ABI struct by value, several declarators or declarations per line, one-dimensional arrays sized by an integer or an
    earlier macro) and raises on anything else (another type, a union, a bit-field, a nested struct, a second dimension,
    an unknown size, a macro that is an expression) instead of guessing."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts, structs = {}, {}
    for item in _ABI_ITEM.finditer(text):
        macro, value, kind, body, name = item.groups()
        if macro is not None:
            if not value and re.search(r"#[ \t]*ifndef[ \t]+%s\s*$" % macro, text[:item.start()]):
                continue                                  # the include guard
            if not re.fullmatch(r"0|[1-9][0-9]*|0[xX][0-9a-fA-F]+", value):
                raise HnError(f"{macro}: the macro's value '{value}' is not an integer literal")
            consts[macro] = int(value, 0)
            continue
        if kind != "struct":
            raise HnError(f"{name}: a typedef of a {kind}, not of a struct")
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            m = re.fullmatch(r"(?:const )?(\w+)( |(?: ?\* ?(?:const ?)?)+)(\w[^*]*)", decl)
            if m is None or ("*" in decl and "," in decl):
                raise HnError(f"{name}: declaration '{decl}' has a form the binding does not know")
            base = C.c_void_p if "*" in decl else _FIELD_SCALARS.get(m.group(1)) or structs.get(m.group(1))
            if base is None:
                raise HnError(f"{name}: declaration '{decl}' has a type the binding does not know")
            for declarator in m.group(3).split(","):
                d = re.fullmatch(r" ?(\w+) ?(?:\[ ?(\w+) ?\])? ?", declarator)
                if d is None:
                    raise HnError(f"{name}: declaration '{decl}' has a form the binding does not know")
                field, size = d.groups()
                if size is None:
                    fields.append((field, base))
                elif size.isdigit() or size in consts:
                    fields.append((field, base * (int(size) if size.isdigit() else consts[size])))
                else:
                    raise HnError(f"{name}: declaration '{decl}' has an array size the binding does not know")
        structs[name] = type(name, (C.Structure,), {"_fields_": fields})
    return consts, structs


# entry points, ABI structs and constants all come from the header the library is compiled against: nothing to mirror
# here.  Every struct and every macro is a module attribute under its header name (HnMlpArgs, HN_MODE_BF16, ...).
with open(HEADER) as _f:
    _header = _f.read()
ARGTYPES = parse_prototypes(_header)
EXPORTS = list(ARGTYPES)
CONSTANTS, STRUCTS = parse_abi(_header)
globals().update(CONSTANTS)
globals().update(STRUCTS)
# the header's HN_CHUNK_UNITS is only the default of a build-time knob: the library's own value wins, as for the ring above
HN_CHUNK_UNITS = _cfg.get("CHUNK_UNITS", int(os.environ.get("HN_CHUNK_UNITS", CONSTANTS["HN_CHUNK_UNITS"])))
HN_AUXG_MAX = 3      # no macro in the header: a template argument of the machine kernels in csrc/hn_mlp.hip

# numpy views of the table structs (uploaded to the device as raw bytes)
PACK_UNIT_DT = np.dtype(STRUCTS["HnPackUnit"])
PACK_BIAS_DT = np.dtype(STRUCTS["HnPackBias"])
FEAT_DT = np.dtype(STRUCTS["HnFeat"])
DWJOB_DT = np.dtype(STRUCTS["HnDwJob"])
DWREDUCE_DT = np.dtype(STRUCTS["HnDwReduceTile"])
ADAM_RANGE_DT = np.dtype(STRUCTS["HnAdamRange"])

_lib = None


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def needs_build() -> bool:
    if not os.path.exists(PRODUCT_LIB_PATH):
        return True
    t = os.path.getmtime(PRODUCT_LIB_PATH)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(CSRC, h) for h in CSRC_HEADERS] + [HEADER]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 into csrc/libhn_hip.so (cross-compiles without a GPU)."""
    if not force and not needs_build():
        return PRODUCT_LIB_PATH
    out = os.environ.get("HN_BUILD_OUT") or PRODUCT_LIB_PATH      # HN_BUILD_OUT: an A/B variant beside the product library
    cmd = [hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics", "-fPIC", "-shared",
           "-o", out] + [os.path.join(CSRC, s) for s in SOURCES]
    for macro in BUILD_MACROS:          # build-time tuning knobs (A/B experiments)
        if os.environ.get(macro):
            cmd.insert(1, f"-D{macro}={os.environ[macro]}")
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise HnError("hipcc failed:\n" + " ".join(cmd) + "\n" + res.stdout + res.stderr)
    if verbose:
        print(res.stdout + res.stderr)
    return out


def build_id() -> dict:
    """Identity of the kernels a measurement was taken on: sha256 over the kernel sources (+ the build-time tuning
    macros in the environment) and over the built library.  bench.py prints it; tools/make_profiles.py stamps the PMC
    traffic summaries with it, and bench.py only quotes a summary whose source hash equals the running build's."""
    import hashlib
    h = hashlib.sha256()
    for d in [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(CSRC, h) for h in CSRC_HEADERS] + [HEADER]:
        with open(d, "rb") as f:
            h.update(f.read())
    for macro in BUILD_MACROS:
        h.update(f"{macro}={os.environ.get(macro, '')};".encode())
    lib = None
    if os.path.exists(LIB_PATH):
        with open(LIB_PATH, "rb") as f:
            lib = hashlib.sha256(f.read()).hexdigest()[:16]
    ident = {"kernel_src_sha256": h.hexdigest()[:16], "lib_sha256": lib}
    if LIB_PATH != PRODUCT_LIB_PATH:      # an A/B variant: the source hash above describes the tree, not this library
        ident["lib_path_override"] = LIB_PATH
        ident["kernel_src_sha256"] = "override:" + (lib or "?")
    if BUILD_CONFIG is not None:
        ident["build_config"] = dict(BUILD_CONFIG)
    return ident


def load():
    """dlopen the library (building it first only if hipcc is around and sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HnError(
            f"{LIB_PATH} is missing: the HIP extension has not been built (run __graft_entry__.build()). "
            "hypernerf_torch_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise HnError(f"{LIB_PATH} does not export {name}")
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = ARGTYPES[name]
    # the host tables in use were cut for the mirrors above: a library built with other knobs must not run under them
    # (e.g. job stages cut for another ring depth or LDS-DMA slot count: garbage gradients, no error)
    buf = (C.c_int32 * len(BUILD_CONFIG_KEYS))()
    n_cfg = lib.hn_build_config(buf, len(BUILD_CONFIG_KEYS))
    now = {k: int(buf[i]) for i, k in enumerate(BUILD_CONFIG_KEYS[:n_cfg])}
    mine = {"WGRAD_STAGES": WGRAD_STAGES, "WGRAD_MAXSLOT": WGRAD_MAXSLOT, "CHUNK_UNITS": HN_CHUNK_UNITS}
    bad = {k: (v, now.get(k)) for k, v in mine.items() if now.get(k) != v}
    if bad:
        raise HnError(f"{LIB_PATH} was built with other tuning knobs than the host tables assume (mirror, library): {bad}; "
                      "re-import hypernerf_torch_amd after building, or unset the HN_* build variables")
    _lib = lib
    return lib


# Optional per-launch timing (bench.py's roofline leg): when KERNEL_TIMES is a dict, every launch made
# through `launch()` is bracketed by HIP events on the launch stream; `collect_kernel_times()` resolves them.
KERNEL_TIMES = None
_PENDING = []
PROF_BUFFER = None   # diagnostic: uint64[8] device tensor receiving in-kernel cycle sums of the MLP machine


def launch(name: str, *args, tag: str = ""):
    """Call one C-ABI entry point on the current stream and check its status."""
    fn = getattr(load(), name)
    if KERNEL_TIMES is None:
        check(fn(*args), name + (f"[{tag}]" if tag else ""))
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = fn(*args)
    e1.record()
    _PENDING.append((name + (f"[{tag}]" if tag else ""), e0, e1))
    check(rc, name)


# Kernel timeline (include/hn_kernels.h, HnMlpArgs.timeline): when TIMELINE is a dict, every launch of the three machine
# kernels is handed a device uint64[8] slot per launch name and times ITSELF — also inside a HIP-graph replay, where no
# host-side event can sit between two kernels.  Enable BEFORE the step is captured (the pointers are baked into the
# graph); `timeline_reset()` zeroes the sums (e.g. after the warm-up), `timeline_read()` returns ms per name.
TIMELINE = None
TIMELINE_TICK_S = 1e-8        # wall_clock64(): 100 MHz


def timeline_slot(name: str, device) -> int:
    if TIMELINE is None:
        return 0
    t = TIMELINE.get(name)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise HnError(f"kernel timeline: first launch of {name} inside a stream capture (run a warm-up step first)")
        t = TIMELINE[name] = torch.zeros(8, dtype=torch.int64, device=device)
    return t.data_ptr()


def timeline_reset():
    torch.cuda.synchronize()
    for t in (TIMELINE or {}).values():
        t.zero_()
    torch.cuda.synchronize()


def timeline_read() -> dict:
    """{launch name: {'ms': summed duration, 'runs': launches, 'span_ms': first start .. last end}} (synchronises)."""
    torch.cuda.synchronize()
    out = {}
    for name, t in (TIMELINE or {}).items():
        v = t.cpu().tolist()
        out[name] = {"ms": v[4] * TIMELINE_TICK_S * 1e3, "runs": int(v[5]), "span_ms": (v[7] - v[6]) * TIMELINE_TICK_S * 1e3,
                     "first_start_tick": v[6], "last_end_tick": v[7]}
    return out


def collect_kernel_times():
    """ms per launch, grouped by name: {name: [ms, ...]} (synchronises)."""
    torch.cuda.synchronize()
    for name, e0, e1 in _PENDING:
        KERNEL_TIMES.setdefault(name, []).append(e0.elapsed_time(e1))
    _PENDING.clear()
    return KERNEL_TIMES


def check(rc: int, what: str):
    if rc != 0:
        kind = "argument error" if rc < 0 else "hipError_t"
        raise HnError(f"{what} failed: {kind} {rc}")


def stream_handle() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HnError("hypernerf_torch_amd runs on MI355X only: got a CPU tensor and there is no CPU fallback "
                          "(the CPU oracle lives in oracle/ and is test infrastructure)")


def ptr(t):
    return None if t is None else t.data_ptr()


def to_device_bytes(arr: np.ndarray, device) -> torch.Tensor:
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    if raw.size == 0:
        raw = np.zeros(16, dtype=np.uint8)
    t = torch.from_numpy(raw.copy()).to(device)
    # tables are uploaded once and then read by launches on WHATEVER stream is current later on: make the upload
    # complete now instead of merely stream-ordered (never inside a stream capture, where the first use has long
    # happened in the warm-up runs)
    if t.is_cuda and not torch.cuda.is_current_stream_capturing():
        torch.cuda.current_stream(t.device).synchronize()
    return t
