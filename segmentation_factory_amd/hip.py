"""ctypes binding of libsegfac_hip.so (the C ABI declared in include/segfac.h).

Only raw device pointers, sizes and the current HIP stream cross this boundary; torch is used
for device memory (caching allocator) and stream handles, never for the arithmetic.  There is no
CPU fallback: if the shared library is missing, or a kernel returns non-zero, a RuntimeError is
raised (the reference's own error convention is Python exceptions).
"""
import ctypes as C
import math
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SEGFAC_HIP_LIB: another build of the same library (same-box A/B of kernel changes, tools/ab_bench.sh); default in-tree
LIB_PATH = os.environ.get('SEGFAC_HIP_LIB') or os.path.join(_HERE, 'libsegfac_hip.so')
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', 'include', 'segfac.h'))
F32, BF16 = 0, 1
ERR_SHAPE = -1          # SEGF_ERR_SHAPE
_lib = None

# ---- the binding is derived from include/segfac.h: its declarations are the only copy of the C ABI ----------------------------
_i, _l, _f, _p = C.c_int, C.c_int64, C.c_float, C.c_void_p
_SCALAR = {'int': _i, 'int32_t': _i, 'int64_t': _l, 'float': _f, 'double': C.c_double}
_POINTEE = {'void', 'char', 'int', 'int32_t', 'int64_t', 'uint8_t', 'uint64_t', 'float'}


def _ctype(ctype, where, structs):
    """ctypes type of one C type of the header ('const' ignored).  Strict: a type outside the rule raises, nothing becomes c_void_p
    by default."""
    t = re.sub(r'\bconst\b', ' ', ctype).replace('*', ' * ').split()
    if t and all(w == '*' for w in t[1:]):
        base, stars = t[0], len(t) - 1
        if stars == 0 and base in _SCALAR:
            return _SCALAR[base]
        if stars == 1 and base == 'char':
            return C.c_char_p
        if stars == 1 and (base in _POINTEE or base in structs):
            return _p
        if stars > 1:
            return C.POINTER(_ctype(base + '*' * (stars - 1), where, structs))
    raise RuntimeError(f'include/segfac.h: {where}: the C type {" ".join(ctype.split())!r} has no ctypes mapping in hip.py')


def _declarators(decl, where, structs):
    """[(name, ctypes type)] of one declaration 'T a, *b, c[3]'."""
    m = re.fullmatch(r'\s*((?:const\s+)?\w+)(.*)', decl, re.S)
    ds = [re.fullmatch(r'\s*(\**)\s*(\w+)\s*(?:\[(\d+)\])?\s*', d) for d in m.group(2).split(',')] if m else [None]
    if not all(ds):
        raise RuntimeError(f'include/segfac.h: {where}: cannot read {" ".join(decl.split())!r}')
    out = []
    for d in ds:
        stars, name, n = d.groups()
        t = _ctype(m.group(1) + stars, f'{where} {name}', structs)
        out.append((name, t * int(n) if n else t))
    return out


def _parse_header(text):
    """({entry point: (restype, [argtypes])}, {typedef name: ctypes.Structure}) of every declaration, as a C compiler reads the header.
    Anything at file scope other than a `typedef struct` or a segf_* function declaration raises."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'#ifdef __cplusplus.*?#endif', ' ', text, flags=re.S)       # the extern "C" wrapper
    text = re.sub(r'^\s*#.*$', ' ', text, flags=re.M)
    structs, decls = {}, {}

    def struct(m):
        fields = [f for d in m.group(1).split(';') if d.strip() for f in _declarators(d, m.group(2), structs)]
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {'_fields_': fields, '__doc__': f'{m.group(2)} of include/segfac.h'})
        return ';'
    text = re.sub(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', struct, text, flags=re.S)
    for stmt in filter(str.strip, text.split(';')):
        m = re.fullmatch(r'\s*(.*?)\b(segf_\w+)\s*\((.*)\)\s*', stmt, re.S)
        if not m:
            raise RuntimeError(f'include/segfac.h: cannot read the declaration {" ".join(stmt.split())!r}')
        ret, name, args = m.groups()
        res = None if ret.split() == ['void'] else _ctype(ret, name, structs)
        decls[name] = (res, [] if args.split() == ['void'] else
                       [t for a in args.split(',') for _, t in _declarators(a, name, structs)])
    return decls, structs


def _read_header():
    if not os.path.isfile(HEADER_PATH):
        raise RuntimeError(f'{HEADER_PATH} is missing: the ctypes binding of libsegfac_hip.so is derived from it; use the package '
                           f'from the repository tree (include/ next to segmentation_factory_amd/).')
    with open(HEADER_PATH) as fh:
        return _parse_header(fh.read())


_DECLS, _STRUCTS = _read_header()
SegfPrepItem = _STRUCTS['SegfPrepItem']                 # one job of segf_prep_grouped
SegfDwItem = _STRUCTS['SegfDwItem']                     # one layer of segf_gemm_dw_db_grouped
SegfFinalizeItem = _STRUCTS['SegfFinalizeItem']         # one member of segf_colreduce_finalize_grouped
InputSample = _STRUCTS['segf_input_sample']             # one image of segf_input_train (72 bytes)
# one image of segf_input_train_scaled (80 bytes).  Kept under its own name, outside _STRUCTS: tests/test_host_cpu.py fixes the
# membership of that table; tests/test_input_scale_cpu.py checks this record's layout against the C compiler the same way.
InputScaledSample = _STRUCTS.pop('segf_input_scaled_sample')


def lib():
    """Load the shared library (once).  Raises if it has not been built -- never falls back."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                f'or `make -C segmentation_factory_amd/csrc`. There is no CPU/eager fallback.')
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _DECLS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def exported_symbols():
    return sorted(_DECLS)


# ---- dispatch policy (csrc/policy.h; documented in include/segfac.h) and launch trace -------------------------------------------
_NO_SUCH = -2 ** 31


def policy(name):
    """Current value of one dispatch switch (field name 'gemm_no_narrow' or environment name 'SEGFAC_GEMM_NO_NARROW').  The library
    reads the environment once, at first use; `policy_set` / `policy_reload` change it afterwards."""
    v = lib().segf_policy_get(name.encode())
    if v == _NO_SUCH:
        raise KeyError(f'no dispatch switch named {name!r} (csrc/policy.h)')
    return v


def policy_set(name, value):
    prev = lib().segf_policy_set(name.encode(), int(value))
    if prev == _NO_SUCH:
        raise KeyError(f'no dispatch switch named {name!r} (csrc/policy.h)')
    return prev


def policy_reload():
    """Re-read every switch from the environment (after os.environ / monkeypatch.setenv changed it)."""
    lib().segf_policy_reload()


def policy_table():
    """[(field, environment name, value, default, description)] of every switch."""
    out = []
    for i in range(lib().segf_policy_count()):
        f, e, d = C.c_char_p(), C.c_char_p(), C.c_char_p()
        v, df = _i(), _i()
        _chk(lib().segf_policy_describe(i, C.byref(f), C.byref(e), C.byref(v), C.byref(df), C.byref(d)), 'segf_policy_describe')
        out.append((f.value.decode(), e.value.decode(), v.value, df.value, d.value.decode()))
    return out


class policy_override:
    """with policy_override(gemm_no_narrow=1): ...   (tests, A/B scripts)"""

    def __init__(self, **kw):
        self.kw, self.prev = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.prev[k] = policy_set(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            policy_set(k, v)
        return False


class trace:
    """Names of the kernels the library launches on this thread inside the block (instantiated names, template arguments included):
    `with hip.trace() as t: hip.gemm(...)` -> t.kernels.  dry_run=True records the decisions WITHOUT launching (no GPU needed; the
    entry points are then called through lib() with placeholder pointers, see tests/test_host_cpu.py)."""

    def __init__(self, dry_run=False, cap=1 << 16):
        self.dry, self.cap, self.kernels, self.launches = dry_run, cap, [], 0

    def __enter__(self):
        lib().segf_trace_begin(int(self.dry))
        return self

    def __exit__(self, *exc):
        buf = C.create_string_buffer(self.cap)
        self.launches = lib().segf_trace_end(buf, self.cap)
        self.kernels = [l for l in buf.value.decode().split('\n') if l]
        return False


def dt_of(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f'unsupported activation dtype {t.dtype}')


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(rc, name):
    if rc != 0:
        raise RuntimeError(f'{name} failed with code {rc} '
                           f'({"argument error" if rc < 0 else "hipError_t"})')


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('segmentation_factory_amd kernels need device tensors (no CPU fallback)')


def _f32(n, device):
    return torch.empty(max(int(n), 1), dtype=torch.float32, device=device)


# ---- plumbing ------------------------------------------------------------------------------
def cast(src: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    _need_cuda(src)
    src = src.contiguous()
    if src.dtype == dtype:
        return src
    dst = torch.empty(src.shape, dtype=dtype, device=src.device)
    _chk(lib().segf_cast(_ptr(src), dt_of(src), _ptr(dst), BF16 if dtype == torch.bfloat16 else F32,
                         src.numel(), _stream()), 'segf_cast')
    return dst


def cast_into(src: torch.Tensor, dst: torch.Tensor):
    """dst.flat[i] = src.flat[i] with dtype conversion, both contiguous (one launch; dst is reused across graph replays)."""
    _need_cuda(src, dst)
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
    _chk(lib().segf_cast(_ptr(src), dt_of(src), _ptr(dst), dt_of(dst), src.numel(), _stream()), 'segf_cast')
    return dst


def cast2d(src: torch.Tensor, dst: torch.Tensor):
    """dst[r, c] = src[r, c] with dtype conversion; both 2-D with unit inner stride (any row stride), or 1-D."""
    _need_cuda(src, dst)
    if src.ndim == 1:
        src, dst = src.view(1, -1) if src.stride(0) == 1 else src.unsqueeze(1), dst.view(1, -1) if dst.stride(0) == 1 else dst.unsqueeze(1)
    rows, cols = src.shape
    assert tuple(dst.shape) == (rows, cols) and (cols == 1 or (src.stride(1) == 1 and dst.stride(1) == 1))
    _chk(lib().segf_cast2d(_ptr(src), dt_of(src), src.stride(0), _ptr(dst), dt_of(dst), dst.stride(0), rows, cols, _stream()),
         'segf_cast2d')
    return dst


def permute021(x: torch.Tensor, A: int, Bd: int, Cd: int, out_dtype: torch.dtype, ld_out=None, out=None) -> torch.Tensor:
    """out[a][c][b] = in[a][b][c]; last dim zero-padded to ld_out.  out: optional contiguous destination of A * Cd * ld_out elements."""
    _need_cuda(x)
    ld_out = Bd if ld_out is None else ld_out
    if out is None:
        out = torch.empty((A, Cd, ld_out), dtype=out_dtype, device=x.device)
    else:
        assert out.is_contiguous() and out.numel() == A * Cd * ld_out and out.dtype == out_dtype
    _chk(lib().segf_permute021(_ptr(x), dt_of(x), _ptr(out), BF16 if out_dtype == torch.bfloat16 else F32,
                               A, Bd, Cd, ld_out, _stream()), 'segf_permute021')
    return out


def _as2d(src, dst):
    if src is not None and src.ndim == 1:
        src = src.view(1, -1) if src.stride(0) == 1 else src.unsqueeze(1)
    if dst.ndim == 1:
        dst = dst.view(1, -1) if dst.stride(0) == 1 else dst.unsqueeze(1)
    return src, dst


def prep_grouped(jobs):
    """Several small layout jobs in one launch (segf_prep_grouped); jobs must be independent of each other:
        ('cast', src, dst)                        dst[r, c] = src[r, c] (2-D with unit inner stride or a column, or 1-D), as cast2d
        ('zero', dst)                             dst[r, c] = 0
        ('perm', src, dst, A, Bd, Cd, ld_out[, a_stride])   dst[a][c][b] = src[a][b][c], last dim zero-padded to ld_out, as permute021;
                                                  a_stride: element distance between the out[a] blocks (rows of a wider matrix)"""
    if not jobs:
        return
    arr = (SegfPrepItem * len(jobs))()
    for k, job in enumerate(jobs):
        it = arr[k]
        it.pb = it.pc = it.ld_src = it.cols = 0
        it.reserved = 0
        if job[0] == 'perm':
            _, src, dst, A, Bd, Cd, ld_out = job[:7]
            astride = job[7] if len(job) > 7 else 0          # optional: distance between consecutive out[a] blocks (default Cd * ld_out)
            _need_cuda(src, dst)
            assert src.is_contiguous() and src.numel() == A * Bd * Cd
            if astride:
                assert astride >= Cd * ld_out and dst.ndim == 2 and dst.shape[0] == A and dst.stride(0) == astride and dst.stride(1) == 1
            else:
                assert dst.is_contiguous() and dst.numel() == A * Cd * ld_out
            it.op, it.src, it.dst, it.rows, it.pb, it.pc, it.ld_dst = 1, src.data_ptr(), dst.data_ptr(), A, Bd, Cd, ld_out
            it.cols = astride
            it.src_dt, it.dst_dt = dt_of(src), dt_of(dst)
        elif job[0] == 'cast':
            src, dst = _as2d(job[1], job[2])
            _need_cuda(src, dst)
            rows, cols = src.shape
            assert tuple(dst.shape) == (rows, cols) and (cols == 1 or (src.stride(1) == 1 and dst.stride(1) == 1)), (src.shape, dst.shape)
            it.op, it.src, it.dst, it.rows, it.cols = 0, src.data_ptr(), dst.data_ptr(), rows, cols
            it.ld_src, it.ld_dst, it.src_dt, it.dst_dt = max(src.stride(0), 1), max(dst.stride(0), 1), dt_of(src), dt_of(dst)
        else:
            assert job[0] == 'zero'
            _, dst = _as2d(None, job[1])
            _need_cuda(dst)
            rows, cols = dst.shape
            assert cols == 1 or dst.stride(1) == 1
            it.op, it.src, it.dst, it.rows, it.cols, it.ld_dst = 2, None, dst.data_ptr(), rows, cols, max(dst.stride(0), 1)
            it.src_dt = it.dst_dt = dt_of(dst)
    _chk(lib().segf_prep_grouped(len(jobs), C.cast(arr, C.c_void_p), _stream()), 'segf_prep_grouped')


def scale_rows(x: torch.Tensor, scale: torch.Tensor, rows_per_group: int) -> torch.Tensor:
    _need_cuda(x, scale)
    rows, cols = x.shape
    y = torch.empty((rows, cols), dtype=x.dtype, device=x.device)
    _chk(lib().segf_scale_rows(dt_of(x), _ptr(x), x.stride(0), _ptr(y), cols, _ptr(scale), rows, cols,
                               rows_per_group, _stream()), 'segf_scale_rows')
    return y


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _need_cuda(a, b)
    rows, cols = a.shape
    y = torch.empty((rows, cols), dtype=a.dtype, device=a.device)
    _chk(lib().segf_add(dt_of(a), _ptr(a), a.stride(0), _ptr(b), b.stride(0), _ptr(y), cols, rows, cols, _stream()),
         'segf_add')
    return y


def colsum(x: torch.Tensor, out=None) -> torch.Tensor:
    _need_cuda(x)
    rows, cols = x.shape
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.numel() == cols and out.is_contiguous()
    ws = _f32(lib().segf_colsum_ws(rows, cols), x.device)
    _chk(lib().segf_colsum(dt_of(x), _ptr(x), x.stride(0), rows, cols, _ptr(out), _ptr(ws), _stream()), 'segf_colsum')
    return out


# ---- GEMM ------------------------------------------------------------------------------------
def gemm(layout: int, A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int, out=None, out_dtype=None, bias=None,
         residual=None, rscale=None, rows_per_group=1, split_k=1) -> torch.Tensor:
    """C[M,N] = A(m,k) B(k,n) (+bias) (residual + rscale * .).  A, B: 2-D tensors with unit inner stride."""
    _need_cuda(A, B)
    assert A.stride(-1) == 1 and B.stride(-1) == 1
    dt = dt_of(A)
    assert dt_of(B) == dt
    out_dtype = out_dtype or A.dtype
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=A.device)
    assert out.stride(-1) == 1
    ws = None
    if split_k > 1:
        ws = _f32(split_k * M * N, A.device)
    _chk(_timed(('gemm', layout, M, N, K), lambda: lib().segf_gemm(
        dt, layout, M, N, K, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(out), dt_of(out), out.stride(0), _ptr(bias),
        _ptr(residual), residual.stride(0) if residual is not None else 0, _ptr(rscale), rows_per_group, split_k, _ptr(ws),
        _stream())), 'segf_gemm')
    return out


def gemm_dw_db(dy: torch.Tensor, x: torch.Tensor, M: int, N: int, K: int, split_k=1, out=None, db_out=None):
    """(dW [M,N] fp32, db [M] fp32) = (dy^T x, column sums of dy) in one pass over dy [K,M]; x is [K,N]."""
    _need_cuda(dy, x)
    assert dy.stride(-1) == 1 and x.stride(-1) == 1 and dt_of(dy) == dt_of(x)
    dw = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=dy.device)
    assert dw.stride(-1) == 1
    db = db_out if db_out is not None else torch.empty(M, dtype=torch.float32, device=dy.device)
    assert db.dtype == torch.float32 and db.numel() == M and db.is_contiguous()
    ws = _f32(lib().segf_gemm_dw_db_ws(M, N, K, split_k), dy.device)
    _chk(_timed(('gemm', 2, M, N, K), lambda: lib().segf_gemm_dw_db(
        dt_of(dy), M, N, K, _ptr(dy), dy.stride(0), _ptr(x), x.stride(0), _ptr(dw), dt_of(dw), dw.stride(0), split_k, _ptr(ws),
        _ptr(db), _stream())), 'segf_gemm_dw_db')
    return dw, db


def gemm_dw_db_grouped(items, shared_split=False):
    """items: [(dy [K, M], x [K, N], M, N, K, split_k, dw fp32 [M, N] view, db fp32 [M])]: the weight + bias gradients of several Linear
    layers in ONE C-ABI call (grouped launches where the shapes allow; each result bitwise equal to gemm_dw_db's)."""
    if not items:
        return
    arr = (SegfDwItem * len(items))()
    keep = []
    dt = None
    for k, (dy, x, M, N, K, split_k, dw, db) in enumerate(items):
        _need_cuda(dy, x, dw, db)
        assert dy.stride(-1) == 1 and x.stride(-1) == 1 and dw.stride(-1) == 1 and dt_of(dy) == dt_of(x)
        assert dw.dtype == torch.float32 and db.dtype == torch.float32 and db.numel() == M and db.is_contiguous()
        dt = dt_of(dy) if dt is None else dt
        assert dt_of(dy) == dt
        ws = _f32(lib().segf_gemm_dw_db_ws(M, N, K, split_k), dy.device)
        keep.append(ws)
        it = arr[k]
        it.M, it.N, it.K = M, N, K
        it.dy, it.lddy, it.x, it.ldx = dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0)
        it.dw, it.lddw, it.db, it.ws, it.split_k, it.shared_split = dw.data_ptr(), dw.stride(0), db.data_ptr(), ws.data_ptr(), split_k, int(shared_split)
    _chk(lib().segf_gemm_dw_db_grouped(dt, len(items), C.cast(arr, C.c_void_p), _stream()), 'segf_gemm_dw_db_grouped')


def gemm_pro_supported(dtype, layout, M, N, K, rows_per_group):
    return bool(lib().segf_gemm_pro_supported(BF16 if dtype == torch.bfloat16 else F32, layout, M, N, K, rows_per_group))


def bn_affine_table(mean, rstd, gamma, beta, chan_scale, groups, Cc):
    """(scale, shift) fp32 [groups, C]: BatchNorm (+ Dropout2d channel scale) as the affine segf_gemm_pro applies."""
    _need_cuda(mean, rstd, gamma, beta)
    scale = torch.empty((groups, Cc), dtype=torch.float32, device=mean.device)
    shift = torch.empty_like(scale)
    _chk(lib().segf_bn_affine_table(_ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(chan_scale), groups, Cc, _ptr(scale),
                                    _ptr(shift), _stream()), 'segf_bn_affine_table')
    return scale, shift


def gemm_pro(layout, A, B, M, N, K, scale, shift, rows_per_group, act, bias=None, split_k=1, out=None):
    """segf_gemm with the activation operand read as act(x * scale[g] + shift[g]) (layout 0: A, bf16 out; layout 2: B, fp32 out)."""
    _need_cuda(A, B, scale, shift)
    assert A.stride(-1) == 1 and B.stride(-1) == 1
    if out is None:
        out = torch.empty((M, N), dtype=A.dtype if layout == 0 else torch.float32, device=A.device)
    ws = _f32(split_k * M * N, A.device) if split_k > 1 else None
    _chk(_timed(('gemm', layout, M, N, K), lambda: lib().segf_gemm_pro(
        dt_of(A), layout, M, N, K, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(out), dt_of(out), out.stride(0), _ptr(bias),
        split_k, _ptr(ws), _ptr(scale), _ptr(shift), rows_per_group, act, _stream())), 'segf_gemm_pro')
    return out


def quant_rows_fp8(x):
    """(q uint8 [rows, K] of e4m3fn bytes, scale fp32 [rows]): row-wise dynamic quantisation, x = q * scale."""
    _need_cuda(x)
    assert x.ndim == 2 and x.stride(1) == 1
    rows, K = x.shape
    q = torch.empty((rows, K), dtype=torch.uint8, device=x.device)
    scale = torch.empty(rows, dtype=torch.float32, device=x.device)
    _chk(lib().segf_quant_rows_fp8(dt_of(x), rows, K, _ptr(x), x.stride(0), _ptr(q), K, _ptr(scale), _stream()), 'segf_quant_rows_fp8')
    return q, scale


def quant_tensor_fp8(x, e5m2=False):
    """(q uint8 [rows, cols], scale fp32 [1]): one dynamic scale for the whole tensor, x = q * scale; e4m3fn or e5m2 bytes."""
    _need_cuda(x)
    assert x.ndim == 2 and x.stride(1) == 1
    rows, cols = x.shape
    q = torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    scale = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = torch.empty(1, dtype=torch.int32, device=x.device)
    _chk(lib().segf_quant_tensor_fp8(dt_of(x), int(e5m2), rows, cols, _ptr(x), x.stride(0), _ptr(q), cols, _ptr(scale), _ptr(ws),
                                     _stream()), 'segf_quant_tensor_fp8')
    return q, scale


def conv3x3_fp8_supported(mode, B, H, W, Cin, Cout):
    return bool(lib().segf_conv3x3_fp8_supported(mode, B, H, W, Cin, Cout))


def conv3x3_fp8(mode, xq, sx, wq, sw, B, H, W, Cin, Cout):
    """mode 0: y [P, Cout] bf16 from xq [P, Cin] e4m3 and wq [Cout, 9 Cin] e4m3; mode 1: dx [P, Cin] from gq [P, Cout] e5m2 and
    wq [Cin, 9 Cout] e4m3.  sx: tensor scale [1]; sw: one scale per weight row."""
    _need_cuda(xq, wq)
    assert xq.dtype == torch.uint8 and wq.dtype == torch.uint8 and xq.stride(-1) == 1 and wq.stride(-1) == 1
    P = B * H * W
    out = torch.empty((P, Cout if mode == 0 else Cin), dtype=torch.bfloat16, device=xq.device)
    key = ('conv3x3_fp8', mode, P, Cin, Cout)
    _chk(_timed(key, lambda: lib().segf_conv3x3_fp8(mode, B, H, W, Cin, Cout, _ptr(xq), xq.stride(0), _ptr(sx), _ptr(wq), wq.stride(0),
                                                    _ptr(sw), _ptr(out), out.stride(0), _stream())), 'segf_conv3x3_fp8')
    return out


_G8_FP8_STAGGER = None


def autotune_gemm8_fp8(force=False):
    """Pick the schedule of the fp8 eight-phase GEMM (segf_gemm8_option) for THIS device, once per process.  The staggered schedule needs
    26 % fewer cycles, but under it some MI355X devices drop their clock from 2.4 to about 1.5 GHz and finish later than with the
    lockstep schedule (UPerHead bottleneck conv, batch 32: 8.3 ms on devices that hold their clock, 12.7 ms on those that do not,
    10.9 ms in lockstep on both) -- so both are timed here under sustained load (about 0.1 s) and the faster one is kept.
    SEGFAC_G8_STAGGER=0/1 skips the measurement.  Never called while a stream is capturing."""
    global _G8_FP8_STAGGER
    if _G8_FP8_STAGGER is not None and not force:
        return _G8_FP8_STAGGER
    forced = policy('g8_stagger')
    if forced >= 0:
        _G8_FP8_STAGGER = int(forced != 0)
        lib().segf_gemm8_option(0, _G8_FP8_STAGGER)
        return _G8_FP8_STAGGER
    if torch.cuda.is_current_stream_capturing():
        return int(lib().segf_gemm8_option(0, -1))
    B, H, W, Cin, Cout = 8, 128, 128, 3072, 768
    dev = torch.device('cuda', torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(0)
    xq = torch.randint(0, 120, (B * H * W, Cin), dtype=torch.uint8, device=dev, generator=g)       # e4m3 bytes: finite values of mixed magnitude
    wq = torch.randint(0, 120, (Cout, 9 * Cin), dtype=torch.uint8, device=dev, generator=g)
    sx = torch.ones(1, device=dev)
    sw = torch.ones(Cout, device=dev)
    times = {0: [], 1: []}
    for rnd in range(2):
        for st in (1, 0):
            lib().segf_gemm8_option(0, st)
            conv3x3_fp8(0, xq, sx, wq, sw, B, H, W, Cin, Cout)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(8):
                conv3x3_fp8(0, xq, sx, wq, sw, B, H, W, Cin, Cout)
            e1.record()
            torch.cuda.synchronize()
            times[st].append(e0.elapsed_time(e1) / 8)
    _G8_FP8_STAGGER = int(min(times[1]) <= min(times[0]))
    lib().segf_gemm8_option(0, _G8_FP8_STAGGER)
    if os.environ.get('SEGFAC_VERBOSE'):
        print(f'[segfac] fp8 eight-phase GEMM: staggered {min(times[1]):.3f} ms, lockstep {min(times[0]):.3f} ms -> stagger = {_G8_FP8_STAGGER}')
    return _G8_FP8_STAGGER


def conv3x3_fp8_wgrad_supported(B, H, W, Cin, Cout):
    return bool(lib().segf_conv3x3_fp8_wgrad_supported(B, H, W, Cin, Cout))


def conv3x3_fp8_wgrad(xq, sx, gq, sg, B, H, W, Cin, Cout):
    """dW fp32 [Cout, 9 Cin] of the 3x3 convolution from the quantised input xq [P, Cin] (e4m3, scale sx) and the quantised output
    gradient gq [P, Cout] (e5m2, scale sg)."""
    _need_cuda(xq, gq)
    assert xq.dtype == torch.uint8 and gq.dtype == torch.uint8 and xq.stride(-1) == 1 and gq.stride(-1) == 1
    P = B * H * W
    out = torch.empty((Cout, 9 * Cin), dtype=torch.float32, device=xq.device)
    sk = pick_splitk(Cout, 9 * Cin, P)
    ws = _f32(sk * Cout * 9 * Cin, xq.device) if sk > 1 else None
    key = ('conv3x3_fp8_wgrad', P, Cin, Cout)
    _chk(_timed(key, lambda: lib().segf_conv3x3_fp8_wgrad(B, H, W, Cin, Cout, _ptr(xq), xq.stride(0), _ptr(sx), _ptr(gq), gq.stride(0), _ptr(sg),
                                                          _ptr(out), out.stride(0), sk, _ptr(ws) if ws is not None else None, _stream())),
         'segf_conv3x3_fp8_wgrad')
    return out


def linear_fp8_supported(mode, M, N, K):
    """mode 0 / 1: y [M, N] from [M, K] x [N, K]; mode 2: the weight gradient [N, K] over M tokens."""
    return bool(lib().segf_linear_fp8_supported(mode, M, N, K))


def linear_fp8(mode, aq, sa, bq, sb, bias=None, residual=None, rscale=None, rows_per_group=1):
    """bf16 [M, N] = sa * sb[None, :] * (aq . bq^T) (+ bias) (residual + rscale * .): aq [M, K] e4m3 (mode 0) or e5m2 (mode 1) with ONE
    scale sa [1], bq [N, K] e4m3 with a scale per row."""
    _need_cuda(aq, bq)
    assert aq.dtype == torch.uint8 and bq.dtype == torch.uint8 and aq.stride(-1) == 1 and bq.stride(-1) == 1
    M, K = aq.shape
    N = bq.shape[0]
    out = torch.empty((M, N), dtype=torch.bfloat16, device=aq.device)
    key = ('linear_fp8', mode, M, N, K)
    _chk(_timed(key, lambda: lib().segf_linear_fp8(mode, M, N, K, _ptr(aq), aq.stride(0), _ptr(sa), _ptr(bq), bq.stride(0), _ptr(sb),
                                                   _ptr(out), N, _ptr(bias), _ptr(residual),
                                                   residual.stride(0) if residual is not None else 0, _ptr(rscale), rows_per_group,
                                                   _stream())), 'segf_linear_fp8')
    return out


def linear_fp8_wgrad(gq, sg, xq, sx, out=None):
    """dW fp32 [N, K] = sg * sx * gq^T xq from the e5m2 gradient gq [T, N] and the e4m3 input xq [T, K] (tensor scales)."""
    _need_cuda(gq, xq)
    assert gq.dtype == torch.uint8 and xq.dtype == torch.uint8 and gq.stride(-1) == 1 and xq.stride(-1) == 1
    T, N = gq.shape
    K = xq.shape[1]
    if out is None:
        out = torch.empty((N, K), dtype=torch.float32, device=gq.device)
    sk = lib().segf_linear_fp8_wgrad_splitk(N, K, T)
    ws = _f32(sk * N * K, gq.device) if sk > 1 else None
    key = ('linear_fp8_wgrad', T, N, K)
    _chk(_timed(key, lambda: lib().segf_linear_fp8_wgrad(N, K, T, _ptr(gq), gq.stride(0), _ptr(sg), _ptr(xq), xq.stride(0), _ptr(sx),
                                                         _ptr(out), out.stride(0), sk, _ptr(ws), _stream())), 'segf_linear_fp8_wgrad')
    return out


def gemm_fp8_supported(M, N, K):
    return bool(lib().segf_gemm_fp8_supported(M, N, K))


def gemm_fp8(xq, sx, wq, sw, bias=None, residual=None, rscale=None, rows_per_group=1):
    """bf16 [M, N] = (xq . wq^T) * sx[:, None] * sw[None, :] (+ bias) (residual + rscale * .) on the fp8 matrix pipe."""
    _need_cuda(xq, wq)
    M, K = xq.shape
    N = wq.shape[0]
    out = torch.empty((M, N), dtype=torch.bfloat16, device=xq.device)
    _chk(_timed(('gemm_fp8', M, N, K), lambda: lib().segf_gemm_fp8(
        M, N, K, _ptr(xq), xq.stride(0), _ptr(sx), _ptr(wq), wq.stride(0), _ptr(sw), _ptr(bias), _ptr(residual),
        residual.stride(0) if residual is not None else 0, _ptr(rscale), rows_per_group, _ptr(out), N, _stream())), 'segf_gemm_fp8')
    return out


class GraphEvent:
    """A HIP event that may be recorded INSIDE a stream capture as an external event-record node (hipEventRecordExternal) and
    waited on by a stream outside the graph at replay (graph.py).  torch.cuda.Event(external=True) raises on ROCm."""

    def __init__(self):
        h = C.c_void_p()
        _chk(lib().segf_event_create(C.byref(h)), 'segf_event_create')
        self.handle = h

    def record_external(self, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream()
        _chk(lib().segf_event_record(self.handle, s.cuda_stream, 1), 'segf_event_record')

    def record(self, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream()
        _chk(lib().segf_event_record(self.handle, s.cuda_stream, 0), 'segf_event_record')

    def wait(self, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream()
        _chk(lib().segf_stream_wait_event(s.cuda_stream, self.handle), 'segf_stream_wait_event')

    def __del__(self):
        try:
            if self.handle:
                lib().segf_event_destroy(self.handle)
        except Exception:
            pass


class KernelTimer:
    """HIP-event timing of selected launches on the stream they are enqueued on (bench.py's roofline leg).
    Usage: ``with KernelTimer(lambda key: key == ('gemm', 0, M, N, K)) as t: ...; t.summary()``."""
    active = None

    def __init__(self, match):
        self.match, self.events = match, {}

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *a):
        KernelTimer.active = None

    def summary(self):
        torch.cuda.synchronize()
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v)) for k, v in self.events.items()}   # (launches, avg ms)


def _timed(key, fn):
    t = KernelTimer.active
    if t is None or not t.match(key):
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    t.events.setdefault(key, []).append((e0, e1))
    return r


def pick_splitk(M, N, K):
    return lib().segf_gemm_pick_splitk(M, N, K)


def pick_splitk_conv3x3(Cin, Cout, P):
    return lib().segf_conv3x3_pick_splitk(Cin, Cout, P)


# ---- norms ---------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps, patch=None):
    """patch = (log2 W, log2 sr): also returns the output in the patch-major row order of a k = s = sr convolution's im2col matrix,
    [rows / sr^2, sr^2 C] (segf_layernorm_fwd_patch) -> (y, mean, rstd, col)."""
    _need_cuda(x, gamma, beta)
    rows, Cc = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    if patch is not None:
        lw, ls = patch
        col = torch.empty((rows >> (2 * ls), Cc << (2 * ls)), dtype=x.dtype, device=x.device)
        _chk(lib().segf_layernorm_fwd_patch(dt_of(x), rows, Cc, _ptr(x), _ptr(gamma), _ptr(beta), eps, _ptr(y), _ptr(mean), _ptr(rstd),
                                            _ptr(col), lw, ls, _stream()), 'segf_layernorm_fwd_patch')
        return y, mean, rstd, col
    _chk(lib().segf_layernorm_fwd(dt_of(x), rows, Cc, _ptr(x), _ptr(gamma), _ptr(beta), eps, _ptr(y), _ptr(mean),
                                  _ptr(rstd), _stream()), 'segf_layernorm_fwd')
    return y, mean, rstd


def layernorm_linear_fwd_supported(dtype, rows, Cc, N):
    """May Linear(LayerNorm(x)) with C -> N run as one forward pass (segf_layernorm_linear_fwd)?  Shape, size and policy rule of the library
    (SEGFAC_LN_LINEAR_FWD_FUSED)."""
    if dtype not in (torch.bfloat16, torch.float32):
        return False
    return bool(lib().segf_layernorm_linear_fwd_supported(BF16 if dtype == torch.bfloat16 else F32, int(rows), int(Cc), int(N)))


def layernorm_linear_fwd(x, gamma, beta, eps, w, bias, patch=None, keep_y=False):
    """out = Linear(LayerNorm(x)) in one pass, x [rows, C] bf16, w [N, C] bf16, bias fp32 [N] -> (out, mean, rstd, y, col): the LayerNorm output
    is not stored unless asked for -- keep_y: y [rows, C] in token order; patch = (log2 W, log2 sr): col, the same rows in the patch-major order
    of layernorm_fwd(..., patch=)."""
    _need_cuda(x, gamma, beta, w, bias)
    rows, Cc = x.shape
    N = w.shape[0]
    assert w.shape == (N, Cc) and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.is_contiguous() and w.is_contiguous()
    assert bias.dtype == torch.float32 and bias.numel() == N and bias.is_contiguous()
    out = torch.empty((rows, N), dtype=x.dtype, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    y = torch.empty_like(x) if keep_y else None
    col, lw, ls = None, 0, 0
    if patch is not None:
        lw, ls = patch
        col = torch.empty((rows >> (2 * ls), Cc << (2 * ls)), dtype=x.dtype, device=x.device)
    _chk(lib().segf_layernorm_linear_fwd(dt_of(x), rows, Cc, N, _ptr(x), _ptr(gamma), _ptr(beta), eps, _ptr(w), _ptr(bias), _ptr(out), _ptr(mean),
                                         _ptr(rstd), _ptr(y), _ptr(col), lw, ls, _stream()), 'segf_layernorm_linear_fwd')
    return out, mean, rstd, y, col


def zeros(shape, dtype, device):
    """torch.zeros through the library's own fill kernel (keeps framework kernels out of the captured step)."""
    t = torch.empty(shape, dtype=dtype, device=device)
    _need_cuda(t)
    _chk(lib().segf_zero(_ptr(t), t.numel() * t.element_size(), _stream()), 'segf_zero')
    return t


def add_i64_(t, v=1):
    """t += v for an int64 scalar on the device (BatchNorm's num_batches_tracked)."""
    assert t.dtype == torch.int64 and t.numel() == 1 and t.is_cuda
    _chk(lib().segf_add_i64(_ptr(t), int(v), _stream()), 'segf_add_i64')
    return t


def debug_spin(us):
    """Test hook: hold the current stream for `us` microseconds."""
    _chk(lib().segf_debug_spin(int(us), _stream()), 'segf_debug_spin')


def hist_accum_(hist, counts, clear=True):
    """hist (fp32) += counts (int64) element by element, counts cleared: Metrics.update's `self.hist += bincount` (util/metrics.py:27)."""
    _need_cuda(hist, counts)
    assert hist.dtype == torch.float32 and counts.dtype == torch.int64 and hist.numel() == counts.numel()
    assert hist.is_contiguous() and counts.is_contiguous()
    _chk(lib().segf_hist_accum(_ptr(hist), _ptr(counts), hist.numel(), int(clear), _stream()), 'segf_hist_accum')
    return hist


def bernoulli_scale(state, keep_prob, n, row_len):
    """fp32 [n]: 1 / kp with probability kp, else 0, kp = keep_prob[i // row_len]; state = uint64-as-int64 [2] {seed, counter}."""
    _need_cuda(state, keep_prob)
    out = torch.empty(n, dtype=torch.float32, device=state.device)
    _chk(lib().segf_bernoulli_scale(_ptr(state), _ptr(keep_prob), n, row_len, _ptr(out), _stream()), 'segf_bernoulli_scale')
    return out


def colreduce_finalize_grouped(items):
    """items: [(partial fp32 [nblk, n], nblk, n, out fp32 [n][, C])]: the finalize steps of several two-stage reductions in one launch."""
    if not items:
        return
    arr = (SegfFinalizeItem * len(items))()
    for k, item in enumerate(items):
        partial, nblk, n, out = item[:4]
        _need_cuda(partial, out)
        # (out may be the first of several ADJACENT views that together hold n elements: LayerNorm's dgamma | dbeta, a depthwise
        # convolution's dw | db -- the latter with a fifth member C: the [10][C] sums land as dw[C][9], db[C])
        assert partial.dtype == torch.float32 and out.dtype == torch.float32 and partial.numel() >= nblk * n
        arr[k].partial, arr[k].out, arr[k].len, arr[k].nblk = partial.data_ptr(), out.data_ptr(), n, nblk
        arr[k].scatter_c = item[4] if len(item) > 4 else 0
    _chk(lib().segf_colreduce_finalize_grouped(len(items), C.cast(arr, C.c_void_p), _stream()), 'segf_colreduce_finalize_grouped')


def layernorm_bwd(x, dy, gamma, mean, rstd, dgb_out=None, dy2=None, dres=None, defer=False, rscale=None, rows_per_group=1, dy2_patch=None):
    """dgb_out: optional (dgamma, dbeta) fp32 [C] views that are ADJACENT in memory (dbeta == dgamma + C): written in place.
    dy2 / dres: optional fan-in operands, dx = LN_bwd(dy + dy2) + dres (segf_layernorm_bwd_fused).
    defer=True (needs dgb_out): the kernel leaves its per-block partial sums and (dx, finalize item) is returned; the caller passes the
    item to colreduce_finalize_grouped later.
    rscale (fp32 [rows / rows_per_group]): the kernel also writes dxs = dx * rscale[row / rows_per_group] (what scale_rows(dx, ...) gives);
    it is returned as the attribute `dx.scaled` of the first result."""
    rows, Cc = x.shape
    dx = torch.empty_like(x)
    dxs = None
    if rscale is not None and rows < (1 << 22):
        _need_cuda(rscale)
        assert rscale.dtype == torch.float32 and rscale.is_contiguous() and rscale.numel() * rows_per_group >= rows
        dxs = torch.empty_like(x)
    ws = _f32(lib().segf_layernorm_bwd_ws(rows, Cc), x.device)
    # (dy2_patch = (log2 W, log2 sr): dy2 holds the same elements in patch-major row order, [rows / sr^2, sr^2 C])
    assert dres is None or (dres.shape == x.shape and dres.dtype == x.dtype and dres.is_contiguous())
    assert dy2 is None or (dy2.numel() == x.numel() and dy2.dtype == x.dtype and dy2.is_contiguous() and (dy2_patch is not None or dy2.shape == x.shape))
    if dgb_out is not None:
        dg, db = dgb_out
        assert db.data_ptr() == dg.data_ptr() + 4 * Cc and dg.numel() == Cc and db.numel() == Cc
    else:
        assert not defer
        dgb = torch.empty((2, Cc), dtype=torch.float32, device=x.device)
        dg, db = dgb[0], dgb[1]
    lw, ls = dy2_patch if (dy2_patch is not None and dy2 is not None) else (-1, 0)
    _chk(lib().segf_layernorm_bwd_patch(dt_of(x), rows, Cc, _ptr(x), _ptr(dy), _ptr(dy2), _ptr(dres), _ptr(gamma), _ptr(mean),
                                        _ptr(rstd), _ptr(dx), None if defer else dg.data_ptr(), None if defer else db.data_ptr(),
                                        _ptr(ws), _ptr(rscale) if dxs is not None else None, int(rows_per_group), _ptr(dxs), lw, ls,
                                        _stream()), 'segf_layernorm_bwd_patch')
    dx.scaled = dxs
    if defer:
        return dx, (ws, int(lib().segf_layernorm_bwd_blocks(rows, Cc)), 2 * Cc, dg)
    return dx, dg, db


def layernorm_linear_bwd_supported(dtype, rows, Cc, N):
    """May the backward of LayerNorm(C) -> Linear(C, N) run as one pass (segf_layernorm_linear_bwd)?  Shape, size and policy rule of the
    library (SEGFAC_LN_LINEAR_BWD_FUSED)."""
    if dtype not in (torch.bfloat16, torch.float32):
        return False
    return bool(lib().segf_layernorm_linear_bwd_supported(BF16 if dtype == torch.bfloat16 else F32, int(rows), int(Cc), int(N)))


def layernorm_linear_bwd_ex_supported(dtype, rows, Cc, N):
    """layernorm_linear_bwd_supported for the general form (segf_layernorm_linear_bwd_ex): N = C as well as N = 4 C."""
    if dtype not in (torch.bfloat16, torch.float32):
        return False
    return bool(lib().segf_layernorm_linear_bwd_ex_supported(BF16 if dtype == torch.bfloat16 else F32, int(rows), int(Cc), int(N)))


def layernorm_linear_bwd(dh, w1, x, y, gamma, mean, rstd, dres=None, rscale=None, rows_per_group=1, outs=None, defer=False, return_dy=False,
                         beta=None, dy2=None, dy2_patch=None):
    """dh [rows, N] bf16: gradient of Linear(LayerNorm(x)) with w1 [N, C] bf16, y = the saved LayerNorm output.
    y = None (needs beta): the kernel rebuilds the LayerNorm output from x, mean, rstd, gamma, beta (segf_layernorm_linear_bwd_ex); then N = C
    is served too, with dy2 = a second consumer's gradient of the LayerNorm output added to dh w1 (dy2_patch = (log2 W, log2 sr): dy2 in
    patch-major row order, as layernorm_bwd takes it).
    -> (dx, dw1, db1, dgamma, dbeta) with the parameter gradients fp32; `dx.scaled` = dx * rscale[row / rows_per_group] when rscale is given.
    outs = (dw1 [N, C], db1 [N], dgamma [C], dbeta [C]) fp32 targets written in place (dbeta adjacent to dgamma: dbeta == dgamma + C).
    defer=True (needs outs): the kernel leaves its per-workgroup partial sums and (dx, [three finalize items]) is returned; the caller
    passes the items to colreduce_finalize_grouped later.  return_dy: the Linear's data gradient [rows, C] is appended to the result."""
    rows, Cc = x.shape
    N = w1.shape[0]
    _need_cuda(dh, w1, x, gamma, mean, rstd)
    assert dh.shape == (rows, N) and w1.shape == (N, Cc)
    assert all(t.dtype == torch.bfloat16 and t.is_contiguous() for t in (dh, w1, x))
    if y is not None:
        _need_cuda(y)
        assert y.shape == x.shape and y.dtype == torch.bfloat16 and y.is_contiguous() and dy2 is None
    else:
        _need_cuda(beta)
        assert beta is not None and beta.dtype == torch.float32 and beta.numel() == Cc and beta.is_contiguous()
        assert dy2 is None or (dy2.numel() == x.numel() and dy2.dtype == x.dtype and dy2.is_contiguous() and (dy2_patch is not None or dy2.shape == x.shape))
    assert dres is None or (dres.shape == x.shape and dres.dtype == x.dtype and dres.is_contiguous())
    dx = torch.empty_like(x)
    dxs = None
    if rscale is not None:
        _need_cuda(rscale)
        assert rscale.dtype == torch.float32 and rscale.is_contiguous() and rscale.numel() * rows_per_group >= rows
        dxs = torch.empty_like(x)
    dyo = torch.empty_like(x) if return_dy else None
    if outs is not None:
        dw, db1, dg, db = outs
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in outs)
        assert dw.numel() == N * Cc and db1.numel() == N and dg.numel() == Cc and db.numel() == Cc and db.data_ptr() == dg.data_ptr() + 4 * Cc
    else:
        assert not defer
        dw = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
        db1 = torch.empty(N, dtype=torch.float32, device=x.device)
        dgb = torch.empty((2, Cc), dtype=torch.float32, device=x.device)
        dg, db = dgb[0], dgb[1]
    ws = _f32(lib().segf_layernorm_linear_bwd_ws(rows, Cc, N), x.device)
    now = [None] * 4 if defer else [dw.data_ptr(), db1.data_ptr(), dg.data_ptr(), db.data_ptr()]
    if y is not None:
        _chk(lib().segf_layernorm_linear_bwd(dt_of(x), rows, Cc, N, _ptr(dh), _ptr(w1), _ptr(x), _ptr(y), _ptr(dres), _ptr(gamma), _ptr(mean),
                                             _ptr(rstd), _ptr(dx), _ptr(rscale), int(rows_per_group), _ptr(dxs), _ptr(dyo), *now, _ptr(ws),
                                             _stream()), 'segf_layernorm_linear_bwd')
    else:
        lw, ls = dy2_patch if (dy2_patch is not None and dy2 is not None) else (-1, 0)
        _chk(lib().segf_layernorm_linear_bwd_ex(dt_of(x), rows, Cc, N, _ptr(dh), _ptr(w1), _ptr(x), None, _ptr(beta), _ptr(dy2), lw, ls, _ptr(dres),
                                                _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(rscale), int(rows_per_group), _ptr(dxs),
                                                _ptr(dyo), *now, _ptr(ws), _stream()), 'segf_layernorm_linear_bwd_ex')
    dx.scaled = dxs
    if defer:
        nblk = int(lib().segf_layernorm_linear_bwd_blocks(rows))
        items = [(ws, nblk, N * Cc, dw), (ws[nblk * N * Cc:], nblk, N, db1), (ws[nblk * (N * Cc + N):], nblk, 2 * Cc, dg)]
        return (dx, items, dyo) if return_dy else (dx, items)
    return (dx, dw, db1, dg, db, dyo) if return_dy else (dx, dw, db1, dg, db)


def bn_stats(x, running_mean, running_var, momentum, eps):
    rows, Cc = x.shape
    mean = torch.empty(Cc, dtype=torch.float32, device=x.device)
    rstd = torch.empty(Cc, dtype=torch.float32, device=x.device)
    ws = _f32(lib().segf_bn_ws(rows, Cc), x.device)
    _chk(lib().segf_bn_stats(dt_of(x), rows, Cc, _ptr(x), _ptr(mean), _ptr(rstd), _ptr(running_mean), _ptr(running_var),
                             momentum, eps, _ptr(ws), _stream()), 'segf_bn_stats')
    return mean, rstd


def bn_apply(x, mean, rstd, gamma, beta, act, chan_scale, rows_per_sample):
    rows, Cc = x.shape
    y = torch.empty_like(x)
    _chk(lib().segf_bn_apply(dt_of(x), rows, Cc, _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), act,
                             _ptr(chan_scale), rows_per_sample, _ptr(y), _stream()), 'segf_bn_apply')
    return y


def bn_bwd(x, dy, mean, rstd, gamma, beta, act, chan_scale, rows_per_sample, eval_mode):
    rows, Cc = x.shape
    dx = torch.empty_like(x)
    dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device)
    ws = _f32(lib().segf_bn_ws(rows, Cc), x.device)
    _chk(lib().segf_bn_bwd(dt_of(x), rows, Cc, _ptr(x), _ptr(dy), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), act,
                           _ptr(chan_scale), rows_per_sample, int(eval_mode), _ptr(dx), _ptr(dgamma), _ptr(dbeta),
                           _ptr(ws), _stream()), 'segf_bn_bwd')
    return dx, dgamma, dbeta


def bn_cls_bwd_supported(dtype, M, Cc, K, rps):
    return dtype == torch.bfloat16 and bool(lib().segf_bn_cls_bwd_supported(BF16, M, Cc, K, rps))


def bn_cls_bwd(dy, w, x, mean, rstd, gamma, beta, act, chan_scale, rows_per_sample, eval_mode):
    """(dx, dgamma, dbeta) of BatchNorm(+act, +Dropout2d scale) whose output gradient is dy @ w (never materialised).
    dy: [M, K] class gradients (K % 32 == 0, pad columns zero); w: [K, C] bf16 classifier weight; x: [M, C] BatchNorm input."""
    _need_cuda(dy, w, x)
    M, Cc = x.shape
    K = w.shape[0]
    assert dy.shape[0] == M and dy.stride(1) == 1 and dy.stride(0) >= K and w.shape[1] == Cc and w.is_contiguous() and x.is_contiguous()
    dx = torch.empty_like(x)
    dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device)
    ws = _f32(lib().segf_bn_cls_bwd_ws(M, Cc, rows_per_sample), x.device)
    _chk(lib().segf_bn_cls_bwd(BF16, M, Cc, K, _ptr(dy), dy.stride(0), _ptr(w), w.stride(0), _ptr(x), _ptr(mean), _ptr(rstd),
                               _ptr(gamma), _ptr(beta), act, _ptr(chan_scale), rows_per_sample, int(eval_mode), _ptr(dx),
                               _ptr(dgamma), _ptr(dbeta), _ptr(ws), _stream()), 'segf_bn_cls_bwd')
    return dx, dgamma, dbeta


def bn_cls_bwd_dw_supported(dtype, M, Cc, K, rps, C1):
    return dtype == torch.bfloat16 and bool(lib().segf_bn_cls_bwd_dw_supported(BF16, M, Cc, K, rps, C1))


def bn_cls_bwd_dw(dy, w, x, mean, rstd, gamma, beta, act, chan_scale, rows_per_sample, eval_mode, x1):
    """bn_cls_bwd plus the product that the consumer of dx needs next: dG fp32 [C, C1 + 8] = [dx^T x1 | colsum(dx) | 0]
    (segf_bn_cls_bwd_dw; x1: [M, C1] bf16, the stage-1 tokens of the folded SegFormerHead).  -> (dx, dgamma, dbeta, dG)."""
    _need_cuda(dy, w, x, x1)
    M, Cc = x.shape
    K, C1 = w.shape[0], x1.shape[1]
    assert dy.shape[0] == M and dy.stride(1) == 1 and dy.stride(0) >= K and w.shape[1] == Cc and w.is_contiguous() and x.is_contiguous()
    assert x1.shape[0] == M and x1.stride(1) == 1 and x1.dtype == torch.bfloat16
    dx = torch.empty_like(x)
    dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device)
    dG = torch.empty((Cc, C1 + 8), dtype=torch.float32, device=x.device)
    ws = _f32(lib().segf_bn_cls_bwd_dw_ws(M, Cc, rows_per_sample), x.device)
    _chk(lib().segf_bn_cls_bwd_dw(BF16, M, Cc, K, _ptr(dy), dy.stride(0), _ptr(w), w.stride(0), _ptr(x), _ptr(mean), _ptr(rstd),
                                  _ptr(gamma), _ptr(beta), act, _ptr(chan_scale), rows_per_sample, int(eval_mode), _ptr(dx),
                                  _ptr(dgamma), _ptr(dbeta), _ptr(ws), _ptr(x1), x1.stride(0), C1, _ptr(dG), _stream()),
         'segf_bn_cls_bwd_dw')
    return dx, dgamma, dbeta, dG


def bn_cls_bwd_full(dy, w, x, mean, rstd, gamma, beta, act, chan_scale, rows_per_sample, eval_mode, x1=None, want_dwcls=True):
    """bn_cls_bwd with everything that can ride along: dG (when x1 is given, as bn_cls_bwd_dw) and dwcls fp32 [K, C] = the
    classifier's weight gradient dy^T (act(bn(x)) * drop) (act 0 / 1 only).  -> (dx, dgamma, dbeta, dG | None, dwcls | None)."""
    _need_cuda(dy, w, x)
    M, Cc = x.shape
    K = w.shape[0]
    assert dy.shape[0] == M and dy.stride(1) == 1 and dy.stride(0) >= K and w.shape[1] == Cc and w.is_contiguous() and x.is_contiguous()
    assert act in (0, 1) or not want_dwcls
    dx = torch.empty_like(x)
    dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device)
    dG, C1 = None, 0
    if x1 is not None:
        assert x1.shape[0] == M and x1.stride(1) == 1 and x1.dtype == torch.bfloat16
        C1 = x1.shape[1]
        dG = torch.empty((Cc, C1 + 8), dtype=torch.float32, device=x.device)
    dwcls = torch.empty((K, Cc), dtype=torch.float32, device=x.device) if want_dwcls else None
    ws = _f32(lib().segf_bn_cls_bwd_full_ws(M, Cc, K, rows_per_sample), x.device)
    _chk(lib().segf_bn_cls_bwd_full(BF16, M, Cc, K, _ptr(dy), dy.stride(0), _ptr(w), w.stride(0), _ptr(x), _ptr(mean), _ptr(rstd),
                                    _ptr(gamma), _ptr(beta), act, _ptr(chan_scale), rows_per_sample, int(eval_mode), _ptr(dx),
                                    _ptr(dgamma), _ptr(dbeta), _ptr(ws), _ptr(x1) if x1 is not None else None,
                                    x1.stride(0) if x1 is not None else 0, C1, _ptr(dG) if dG is not None else None,
                                    _ptr(dwcls) if dwcls is not None else None, _stream()), 'segf_bn_cls_bwd_full')
    return dx, dgamma, dbeta, dG, dwcls


def bn_cls_bwd_full_db_supported(dtype, M, Cc, K, rps):
    return dtype == torch.bfloat16 and bool(lib().segf_bn_cls_bwd_full_db_supported(BF16, M, Cc, K, rps))


def bn_cls_bwd_full_db(dy, w, x, mean, rstd, gamma, beta, act, chan_scale, rows_per_sample, eval_mode, x1=None):
    """bn_cls_bwd_full with the classifier's bias gradient dbcls fp32 [K] = colsum(dy) riding on pass 1 as well (segf_bn_cls_bwd_full_db;
    act 0 / 1 only).  -> (dx, dgamma, dbeta, dG | None, dwcls, dbcls); all but dbcls have the bits of bn_cls_bwd_full."""
    _need_cuda(dy, w, x)
    M, Cc = x.shape
    K = w.shape[0]
    assert dy.shape[0] == M and dy.stride(1) == 1 and dy.stride(0) >= K and w.shape[1] == Cc and w.is_contiguous() and x.is_contiguous()
    assert act in (0, 1)
    dx = torch.empty_like(x)
    dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device)
    dG, C1 = None, 0
    if x1 is not None:
        assert x1.shape[0] == M and x1.stride(1) == 1 and x1.dtype == torch.bfloat16
        C1 = x1.shape[1]
        dG = torch.empty((Cc, C1 + 8), dtype=torch.float32, device=x.device)
    dwcls = torch.empty((K, Cc), dtype=torch.float32, device=x.device)
    dbcls = torch.empty(K, dtype=torch.float32, device=x.device)
    ws = _f32(lib().segf_bn_cls_bwd_full_db_ws(M, Cc, K, rows_per_sample), x.device)
    _chk(lib().segf_bn_cls_bwd_full_db(BF16, M, Cc, K, _ptr(dy), dy.stride(0), _ptr(w), w.stride(0), _ptr(x), _ptr(mean), _ptr(rstd),
                                       _ptr(gamma), _ptr(beta), act, _ptr(chan_scale), rows_per_sample, int(eval_mode), _ptr(dx),
                                       _ptr(dgamma), _ptr(dbeta), _ptr(ws), _ptr(x1) if x1 is not None else None,
                                       x1.stride(0) if x1 is not None else 0, C1, _ptr(dG) if dG is not None else None,
                                       _ptr(dwcls), _ptr(dbcls), _stream()), 'segf_bn_cls_bwd_full_db')
    return dx, dgamma, dbeta, dG, dwcls, dbcls


def grn_fwd(x, gamma, beta, B, rps, pre_gelu=False):
    Cc = x.shape[1]
    y = torch.empty_like(x)
    a = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    sq = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    ws = _f32(lib().segf_grn_ws(B, rps, Cc, 0), x.device)
    _chk(lib().segf_grn_fwd(dt_of(x), B, rps, Cc, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(a), _ptr(sq), _ptr(ws),
                            int(pre_gelu), _stream()), 'segf_grn_fwd')
    return y, sq


def grn_bwd(x, dy, gamma, sq, B, rps, pre_gelu=False):
    Cc = x.shape[1]
    dx = torch.empty_like(x)
    dgb = torch.empty((2, Cc), dtype=torch.float32, device=x.device)
    ws = _f32(lib().segf_grn_ws(B, rps, Cc, 1), x.device)
    _chk(lib().segf_grn_bwd(dt_of(x), B, rps, Cc, _ptr(x), _ptr(dy), _ptr(gamma), _ptr(sq), _ptr(dx), dgb[0].data_ptr(),
                            dgb[1].data_ptr(), _ptr(ws), int(pre_gelu), _stream()), 'segf_grn_bwd')
    return dx, dgb[0], dgb[1]


# ---- attention ------------------------------------------------------------------------------------
def attention_fwd(q, k, v, B, heads, N, Nkv, hd, scale):
    """q: [B*N, >=heads*hd] view; k, v: [B*Nkv, ...] views (unit inner stride)."""
    o = torch.empty((B * N, heads * hd), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, heads, N), dtype=torch.float32, device=q.device)
    _chk(lib().segf_attention_fwd(dt_of(q), B, heads, N, Nkv, hd, _ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v),
                                  v.stride(0), scale, _ptr(o), o.stride(0), _ptr(lse), _stream()), 'segf_attention_fwd')
    return o, lse


def attention_bwd(q, k, v, o, d_o, lse, B, heads, N, Nkv, hd, scale, dk, dv):
    """dk / dv are written into caller-provided views (the two halves of the kv-linear gradient)."""
    dq = torch.empty((B * N, heads * hd), dtype=q.dtype, device=q.device)
    ws = _f32(lib().segf_attention_bwd_ws(B, heads, N, Nkv, hd), q.device)
    _chk(lib().segf_attention_bwd(dt_of(q), B, heads, N, Nkv, hd, _ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v),
                                  v.stride(0), scale, _ptr(o), o.stride(0), _ptr(d_o), d_o.stride(0), _ptr(lse),
                                  _ptr(dq), dq.stride(0), _ptr(dk), dk.stride(0), _ptr(dv), dv.stride(0), _ptr(ws),
                                  _stream()), 'segf_attention_bwd')
    return dq


def _group_attention_check(t, B, H, W, heads, G, interval, lda):
    """The refusal happens here, on the host, before any launch: head dim 32 and G * G <= 64 slots per group only."""
    if G * G <= 64 and not lib().segf_group_attention_supported(dt_of(t), B, H, W, heads, 32, G, interval, int(lda)):
        raise RuntimeError(f'group attention: no kernel for a {H} x {W} map, batch {B}, {heads} heads of 32, groups of {G} x {G} '
                           f'({"LDA" if lda else "SDA"}, interval {interval}): sizes must be positive and B * H * W below 2^29')
    if G * G > 64:
        raise RuntimeError(f'group attention: no kernel for groups of {G} x {G} = {G * G} tokens ({"LDA" if lda else "SDA"}, interval '
                           f'{interval}) on a {H} x {W} map, batch {B}, {heads} heads of 32: a group holds at most 64 tokens '
                           f'(there is no fallback path)')


def group_attention_fwd(qkv, bias, B, H, W, heads, G, interval, lda, scale):
    """qkv: [B*H*W, >= 3*heads*32] view (unit inner stride) = [q | k | v]; bias: [heads, G*G, G*G] fp32.  -> (o [B*H*W, heads*32], lse)."""
    _need_cuda(qkv, bias)
    _group_attention_check(qkv, B, H, W, heads, G, interval, lda)
    rows = B * H * W
    assert qkv.shape[0] == rows and qkv.stride(1) == 1 and bias.is_contiguous() and bias.dtype == torch.float32
    assert qkv.shape[1] >= 3 * heads * 32, f'qkv has {qkv.shape[1]} columns, {heads} heads of 32 need {3 * heads * 32}'
    assert tuple(bias.shape) == (heads, G * G, G * G), (tuple(bias.shape), heads, G)
    o = torch.empty((rows, heads * 32), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((heads, rows), dtype=torch.float32, device=qkv.device)
    _chk(lib().segf_group_attention_fwd(dt_of(qkv), B, H, W, heads, 32, G, interval, int(lda), _ptr(qkv), qkv.stride(0), _ptr(bias),
                                        scale, _ptr(o), o.stride(0), _ptr(lse), _stream()), 'segf_group_attention_fwd')
    return o, lse


def group_attention_bwd(qkv, bias, d_o, lse, B, H, W, heads, G, interval, lda, scale):
    """-> (dqkv [B*H*W, 3*heads*32] in qkv's dtype, dbias [heads, G*G, G*G] fp32)."""
    _need_cuda(qkv, bias, d_o)
    _group_attention_check(qkv, B, H, W, heads, G, interval, lda)
    assert qkv.shape[1] >= 3 * heads * 32 and d_o.shape[1] >= heads * 32 and d_o.stride(1) == 1
    dqkv = torch.empty((B * H * W, 3 * heads * 32), dtype=qkv.dtype, device=qkv.device)
    dbias = torch.empty((heads, G * G, G * G), dtype=torch.float32, device=qkv.device)
    ws = _f32(lib().segf_group_attention_bwd_ws(B, H, W, heads, 32, G, interval, int(lda)), qkv.device)
    _chk(lib().segf_group_attention_bwd(dt_of(qkv), B, H, W, heads, 32, G, interval, int(lda), _ptr(qkv), qkv.stride(0), _ptr(bias),
                                        scale, _ptr(d_o), d_o.stride(0), _ptr(lse), _ptr(dqkv), dqkv.stride(0), _ptr(dbias), _ptr(ws),
                                        _stream()), 'segf_group_attention_bwd')
    return dqkv, dbias


# ---- CAS-ViT additive token mixer (csrc/token_mixer.hip) ---------------------------------------------------------------------
def _token_mixer_check(what, supported, B, HW, Cc, *ops):
    """The refusal happens here, on the host, before any launch.  ops: the [rows, >= Cc] operands that may be column slices."""
    for t in ops:
        assert t.ndim == 2 and t.shape[0] == B * HW and t.shape[1] >= Cc and (t.stride(1) == 1 or t.shape[1] == 1), (what, tuple(t.shape))
    if not all(supported(dt_of(ops[0]), B, HW, Cc, ld) for ld in sorted({max(t.stride(0), Cc) if t.shape[0] == 1 else t.stride(0) for t in ops})):
        raise RuntimeError(f'{what}: no kernel for {B} x {HW} rows of {Cc} channels (leading dimensions {[t.stride(0) for t in ops]}): the '
                           f'channel count must be a multiple of 8 and at most 1024, B * HW below 2^29, rows 16-byte aligned '
                           f'(there is no fallback path)')
    for t in ops:
        assert t.data_ptr() % 16 == 0, f'{what}: operand not 16-byte aligned'


def spatial_gate_fwd(x, r, w, B, HW):
    """x: [B*HW, C] (any aligned row stride), r: [B*HW, C] contiguous, w: [C] fp32 -> (y [B*HW, C], s [B*HW] fp32, pool [B, C] fp32)."""
    _need_cuda(x, r, w)
    Cc = w.numel()
    _token_mixer_check('spatial gate', lib().segf_spatial_gate_supported, B, HW, Cc, x, r)
    assert r.is_contiguous() and r.shape[1] == Cc and r.dtype == x.dtype and w.dtype == torch.float32 and w.is_contiguous()
    y = torch.empty((B * HW, Cc), dtype=x.dtype, device=x.device)
    s = torch.empty(B * HW, dtype=torch.float32, device=x.device)
    pool = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    ws = _f32(lib().segf_spatial_gate_fwd_ws(B, HW, Cc), x.device)
    _chk(lib().segf_spatial_gate_fwd(dt_of(x), B, HW, Cc, _ptr(x), x.stride(0), _ptr(r), _ptr(w), _ptr(s), _ptr(y), y.stride(0), _ptr(pool),
                                     _ptr(ws), _stream()), 'segf_spatial_gate_fwd')
    return y, s, pool


def spatial_gate_bwd(dy, dpool, x, r, s, w, B, HW, dx=None):
    """-> (dx [B*HW, C] (or written into the given view), dr [B*HW, C], dw [C] fp32); dpool: [B, C] fp32 or None."""
    _need_cuda(dy, x, r, s, w)
    Cc = w.numel()
    if dx is None:
        dx = torch.empty((B * HW, Cc), dtype=x.dtype, device=x.device)
    _token_mixer_check('spatial gate backward', lib().segf_spatial_gate_supported, B, HW, Cc, dy, x, r, dx)
    assert dpool is None or (dpool.is_contiguous() and dpool.dtype == torch.float32 and tuple(dpool.shape) == (B, Cc))
    assert r.is_contiguous() and s.is_contiguous() and s.numel() == B * HW and dy.dtype == x.dtype == r.dtype == dx.dtype
    dr = torch.empty((B * HW, Cc), dtype=x.dtype, device=x.device)
    dw = torch.empty(Cc, dtype=torch.float32, device=x.device)
    ws = _f32(lib().segf_spatial_gate_bwd_ws(B, HW, Cc), x.device)
    _chk(lib().segf_spatial_gate_bwd(dt_of(x), B, HW, Cc, _ptr(dy), dy.stride(0), _ptr(dpool), _ptr(x), x.stride(0), _ptr(r), _ptr(s),
                                     _ptr(w), _ptr(dx), dx.stride(0), _ptr(dr), _ptr(dw), _ptr(ws), _stream()), 'segf_spatial_gate_bwd')
    return dx, dr, dw


def channel_gate_mix_fwd(q1, k1, gq, gk, B, HW):
    """u = q1 * gq[b] + k1 * gk[b];  gq, gk: [B, C] fp32."""
    _need_cuda(q1, k1, gq, gk)
    Cc = gq.shape[1]
    _token_mixer_check('channel gate mix', lib().segf_channel_gate_mix_supported, B, HW, Cc, q1, k1)
    assert gq.is_contiguous() and gk.is_contiguous() and gq.dtype == gk.dtype == torch.float32 and tuple(gq.shape) == tuple(gk.shape) == (B, Cc)
    assert q1.dtype == k1.dtype
    u = torch.empty((B * HW, Cc), dtype=q1.dtype, device=q1.device)
    _chk(lib().segf_channel_gate_mix_fwd(dt_of(q1), B, HW, Cc, _ptr(q1), q1.stride(0), _ptr(k1), k1.stride(0), _ptr(gq), _ptr(gk), _ptr(u),
                                         u.stride(0), _stream()), 'segf_channel_gate_mix_fwd')
    return u


def channel_gate_mix_bwd(du, q1, k1, gq, gk, B, HW, dq1=None, dk1=None):
    """-> (dq1, dk1 [B*HW, C] (or written into the given views), dgq, dgk [B, C] fp32)."""
    _need_cuda(du, q1, k1, gq, gk)
    Cc = gq.shape[1]
    if dq1 is None:
        dq1 = torch.empty((B * HW, Cc), dtype=q1.dtype, device=q1.device)
    if dk1 is None:
        dk1 = torch.empty((B * HW, Cc), dtype=q1.dtype, device=q1.device)
    _token_mixer_check('channel gate mix backward', lib().segf_channel_gate_mix_supported, B, HW, Cc, du, q1, k1, dq1, dk1)
    assert gq.is_contiguous() and gk.is_contiguous() and du.dtype == q1.dtype == k1.dtype == dq1.dtype == dk1.dtype
    dgq = torch.empty((B, Cc), dtype=torch.float32, device=q1.device)
    dgk = torch.empty((B, Cc), dtype=torch.float32, device=q1.device)
    ws = _f32(lib().segf_channel_gate_mix_bwd_ws(B, HW, Cc), q1.device)
    _chk(lib().segf_channel_gate_mix_bwd(dt_of(q1), B, HW, Cc, _ptr(du), du.stride(0), _ptr(q1), q1.stride(0), _ptr(k1), k1.stride(0),
                                         _ptr(gq), _ptr(gk), _ptr(dq1), dq1.stride(0), _ptr(dk1), dk1.stride(0), _ptr(dgq), _ptr(dgk),
                                         _ptr(ws), _stream()), 'segf_channel_gate_mix_bwd')
    return dq1, dk1, dgq, dgk


def _gated_mul_supported(dt, B, HW, Cc, ld):
    return lib().segf_gated_mul_supported(dt, B * HW, Cc, ld)


def gated_mul_fwd(a, v):
    """z = a * v on [M, C] operands (any aligned row strides)."""
    _need_cuda(a, v)
    M, Cc = a.shape
    _token_mixer_check('gated product', _gated_mul_supported, 1, M, Cc, a, v)
    assert a.dtype == v.dtype and v.shape[1] == Cc
    z = torch.empty((M, Cc), dtype=a.dtype, device=a.device)
    _chk(lib().segf_gated_mul_fwd(dt_of(a), M, Cc, _ptr(a), a.stride(0), _ptr(v), v.stride(0), _ptr(z), z.stride(0), _stream()),
         'segf_gated_mul_fwd')
    return z


def gated_mul_bwd(dz, a, v, da=None, dv=None):
    """-> (da = dz * v, dv = dz * a), written into the given views when there are any."""
    _need_cuda(dz, a, v)
    M, Cc = a.shape
    if da is None:
        da = torch.empty((M, Cc), dtype=a.dtype, device=a.device)
    if dv is None:
        dv = torch.empty((M, Cc), dtype=a.dtype, device=a.device)
    _token_mixer_check('gated product backward', _gated_mul_supported, 1, M, Cc, dz, a, v, da, dv)
    assert dz.dtype == a.dtype == v.dtype == da.dtype == dv.dtype and v.shape[1] == Cc and dz.shape[1] == Cc
    _chk(lib().segf_gated_mul_bwd(dt_of(a), M, Cc, _ptr(dz), dz.stride(0), _ptr(a), a.stride(0), _ptr(v), v.stride(0), _ptr(da),
                                  da.stride(0), _ptr(dv), dv.stride(0), _stream()), 'segf_gated_mul_bwd')
    return da, dv


# ---- MetaFormer / ConvFormer: StarReLU and the residual scale (csrc/metaformer.hip) -----------------------------------------------
def _metaformer_check(what, supported, rows, cols, limit, *ops):
    """The refusal happens here, on the host, before any launch.  ops: the [rows, >= cols] operands that may be column slices."""
    for t in ops:
        assert t.ndim == 2 and t.shape[0] == rows and t.shape[1] >= cols and (t.stride(1) == 1 or t.shape[1] == 1), (what, tuple(t.shape))
        assert t.dtype == ops[0].dtype, (what, t.dtype, ops[0].dtype)
    lds = sorted({max(t.stride(0), cols) if rows == 1 else t.stride(0) for t in ops})
    if not all(supported(dt_of(ops[0]), rows, cols, ld) for ld in lds):
        raise RuntimeError(f'{what}: no kernel for {rows} rows of {cols} columns (leading dimensions {lds}): the column count must be a '
                           f'multiple of 8 and at most {limit}, rows 16-byte aligned, rows * leading dimension below 2^31 '
                           f'(there is no fallback path)')
    for t in ops:
        assert t.data_ptr() % 16 == 0, f'{what}: operand not 16-byte aligned'


def _ld(t, cols):
    return max(t.stride(0), cols) if t.shape[0] == 1 else t.stride(0)


def _one_f32(t, what):
    assert t.is_cuda and t.dtype == torch.float32 and t.numel() == 1, f'{what}: a one-element fp32 device tensor is expected'
    return t


def starrelu_fwd(u, s, b, y=None):
    """y = s * relu(u)^2 + b on [rows, cols] (any aligned row stride); s, b: one-element fp32 device tensors, read by the kernel."""
    _need_cuda(u, s, b)
    rows, cols = u.shape
    if y is None:
        y = torch.empty((rows, cols), dtype=u.dtype, device=u.device)
    _metaformer_check('StarReLU', lib().segf_starrelu_supported, rows, cols, 8192, u, y)
    _chk(lib().segf_starrelu_fwd(dt_of(u), rows, cols, _ptr(u), _ld(u, cols), _ptr(_one_f32(s, 'StarReLU scale')),
                                 _ptr(_one_f32(b, 'StarReLU bias')), _ptr(y), _ld(y, cols), _stream()), 'segf_starrelu_fwd')
    return y


def starrelu_bwd(u, dy, s, du=None, ds=None, db=None):
    """-> (du = dy * 2 s relu(u), ds = sum dy relu(u)^2, db = sum dy); ds, db: fp32 [1] each (written into the given views when there are any)."""
    _need_cuda(u, dy, s)
    rows, cols = u.shape
    if du is None:
        du = torch.empty((rows, cols), dtype=u.dtype, device=u.device)
    _metaformer_check('StarReLU backward', lib().segf_starrelu_supported, rows, cols, 8192, u, dy, du)
    assert dy.shape[1] == cols
    if ds is None:
        ds = torch.empty(1, dtype=torch.float32, device=u.device)
    if db is None:
        db = torch.empty(1, dtype=torch.float32, device=u.device)
    ws = _f32(lib().segf_starrelu_bwd_ws(rows, cols), u.device)
    _chk(lib().segf_starrelu_bwd(dt_of(u), rows, cols, _ptr(u), _ld(u, cols), _ptr(dy), _ld(dy, cols), _ptr(_one_f32(s, 'StarReLU scale')),
                                 _ptr(du), _ld(du, cols), _ptr(_one_f32(ds, 'ds')), _ptr(_one_f32(db, 'db')), _ptr(ws), _stream()),
         'segf_starrelu_bwd')
    return du, ds, db


def colscale_fwd(x, scale, y=None):
    """y = x * scale[c] on [rows, C] (any aligned row stride); scale fp32 [C]."""
    _need_cuda(x, scale)
    rows, Cc = x.shape[0], scale.numel()
    if y is None:
        y = torch.empty((rows, Cc), dtype=x.dtype, device=x.device)
    _metaformer_check('residual scale', lib().segf_colscale_supported, rows, Cc, 2048, x, y)
    assert scale.dtype == torch.float32 and scale.is_contiguous() and scale.data_ptr() % 16 == 0
    _chk(lib().segf_colscale_fwd(dt_of(x), rows, Cc, _ptr(x), _ld(x, Cc), _ptr(scale), _ptr(y), _ld(y, Cc), _stream()), 'segf_colscale_fwd')
    return y


def colscale_bwd(dy, x, scale, dx=None, dscale=None):
    """-> (dx = dy * scale[c], dscale[c] = sum_rows dy * x fp32 [C]), written into the given views when there are any."""
    _need_cuda(dy, x, scale)
    rows, Cc = x.shape[0], scale.numel()
    if dx is None:
        dx = torch.empty((rows, Cc), dtype=x.dtype, device=x.device)
    _metaformer_check('residual scale backward', lib().segf_colscale_supported, rows, Cc, 2048, dy, x, dx)
    assert scale.dtype == torch.float32 and scale.is_contiguous() and scale.data_ptr() % 16 == 0
    if dscale is None:
        dscale = torch.empty(Cc, dtype=torch.float32, device=x.device)
    assert dscale.dtype == torch.float32 and dscale.is_contiguous() and dscale.numel() == Cc
    ws = _f32(lib().segf_colscale_bwd_ws(rows, Cc), x.device)
    _chk(lib().segf_colscale_bwd(dt_of(x), rows, Cc, _ptr(dy), _ld(dy, Cc), _ptr(x), _ld(x, Cc), _ptr(scale), _ptr(dx), _ld(dx, Cc),
                                 _ptr(dscale), _ptr(ws), _stream()), 'segf_colscale_bwd')
    return dx, dscale


# ---- spatial ----------------------------------------------------------------------------------------
def dwconv3x3_gelu_fwd(x, w9, bias, B, H, W, Cc, apply_gelu=True):
    y = torch.empty_like(x)
    _chk(lib().segf_dwconv3x3_gelu_fwd(dt_of(x), B, H, W, Cc, _ptr(x), _ptr(w9), _ptr(bias), int(apply_gelu), _ptr(y),
                                       _stream()), 'segf_dwconv3x3_gelu_fwd')
    return y


def dwconv3x3_gelu_bwd(x, w9, bias, dy, B, H, W, Cc, apply_gelu=True, dw_out=None, db_out=None, defer=False):
    """defer=True (needs dw_out and db_out ADJACENT in memory, db right behind dw): the kernels leave their per-block partial sums and
    (dx, finalize item) is returned; the caller passes the item to colreduce_finalize_grouped later."""
    du = torch.empty_like(x)
    dx = torch.empty_like(x)
    if defer:
        assert dw_out.dtype == db_out.dtype == torch.float32 and dw_out.is_contiguous() and dw_out.numel() == 9 * Cc
        assert db_out.numel() == Cc and db_out.data_ptr() == dw_out.data_ptr() + 36 * Cc
        ws = _f32(lib().segf_dwconv3x3_bwd_ws(B, H, W, Cc), x.device)
        _chk(lib().segf_dwconv3x3_gelu_bwd(dt_of(x), B, H, W, Cc, _ptr(x), _ptr(w9), _ptr(bias), int(apply_gelu), _ptr(dy),
                                           _ptr(du), _ptr(dx), None, None, _ptr(ws), _stream()), 'segf_dwconv3x3_gelu_bwd')
        return dx, (ws, int(lib().segf_dwconv3x3_bwd_blocks(dt_of(x), B, H, W, Cc)), 10 * Cc, dw_out, Cc)
    dw = dw_out if dw_out is not None else torch.empty((Cc, 9), dtype=torch.float32, device=x.device)
    db = db_out if db_out is not None else torch.empty(Cc, dtype=torch.float32, device=x.device)
    assert dw.is_contiguous() and dw.numel() == Cc * 9 and db.is_contiguous() and db.numel() == Cc and dw.dtype == db.dtype == torch.float32
    ws = _f32(lib().segf_dwconv3x3_bwd_ws(B, H, W, Cc), x.device)
    _chk(lib().segf_dwconv3x3_gelu_bwd(dt_of(x), B, H, W, Cc, _ptr(x), _ptr(w9), _ptr(bias), int(apply_gelu), _ptr(dy),
                                       _ptr(du), _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws), _stream()),
         'segf_dwconv3x3_gelu_bwd')
    return dx, dw, db


def dwconv3x3_gelu_bwd_fc2_supported(dtype, B, H, W, Cc, Cin):
    """Does the Mix-FFN backward of this shape take the form that builds fc2's data gradient inside pass A (host arithmetic only)?"""
    dt = BF16 if dtype == torch.bfloat16 else F32
    return bool(lib().segf_dwconv3x3_gelu_bwd_fc2_supported(dt, B, H, W, Cc, Cin))


def dwconv3x3_gelu_bwd_fc2_lds_supported(dtype, B, H, W, Cc, Cin):
    """The same question for C_in = 160 / 256 (MiT stages 3 and 4), the kernel form with fc2's weight fragments in LDS."""
    dt = BF16 if dtype == torch.bfloat16 else F32
    return bool(lib().segf_dwconv3x3_gelu_bwd_fc2_lds_supported(dt, B, H, W, Cc, Cin))


def dwconv3x3_gelu_bwd_fc2(x, w9, bias, dys, w2, B, H, W, Cc, Cin, dw_out=None, db_out=None, defer=False, return_du=False):
    """Backward of gelu(dwconv3x3(x) + bias) -> fc2 from fc2's OUTPUT gradient dys [B*H*W, Cin] and w2 [Cin, Cc] (bf16): what
    gemm(1, dys, w2, M, Cc, Cin) followed by dwconv3x3_gelu_bwd returns, bit for bit, without the [M, Cc] gradient map.  dw_out / db_out /
    defer as in dwconv3x3_gelu_bwd; return_du appends the scratch du (tests)."""
    _need_cuda(x, dys, w2)
    assert x.dtype == dys.dtype == w2.dtype == torch.bfloat16 and x.is_contiguous() and w2.is_contiguous()
    assert dys.shape == (B * H * W, Cin) and dys.stride(1) == 1 and w2.shape == (Cin, Cc)
    du = torch.empty_like(x)
    dx = torch.empty_like(x)
    ws = _f32(lib().segf_dwconv3x3_bwd_ws(B, H, W, Cc), x.device)
    if defer:
        assert dw_out.dtype == db_out.dtype == torch.float32 and dw_out.is_contiguous() and dw_out.numel() == 9 * Cc
        assert db_out.numel() == Cc and db_out.data_ptr() == dw_out.data_ptr() + 36 * Cc
        blocks = int(lib().segf_dwconv3x3_bwd_blocks(dt_of(x), B, H, W, Cc))
        _chk(lib().segf_dwconv3x3_gelu_bwd_fc2(BF16, B, H, W, Cc, Cin, _ptr(x), _ptr(w9), _ptr(bias), _ptr(dys), dys.stride(0), _ptr(w2),
                                               _ptr(du), _ptr(dx), None, None, _ptr(ws), _stream()), 'segf_dwconv3x3_gelu_bwd_fc2')
        out = (dx, (ws, blocks, 10 * Cc, dw_out, Cc))
        return out + (du,) if return_du else out
    dw = dw_out if dw_out is not None else torch.empty((Cc, 9), dtype=torch.float32, device=x.device)
    db = db_out if db_out is not None else torch.empty(Cc, dtype=torch.float32, device=x.device)
    assert dw.is_contiguous() and dw.numel() == Cc * 9 and db.is_contiguous() and db.numel() == Cc and dw.dtype == db.dtype == torch.float32
    _chk(lib().segf_dwconv3x3_gelu_bwd_fc2(BF16, B, H, W, Cc, Cin, _ptr(x), _ptr(w9), _ptr(bias), _ptr(dys), dys.stride(0), _ptr(w2),
                                           _ptr(du), _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws), _stream()), 'segf_dwconv3x3_gelu_bwd_fc2')
    return (dx, dw, db, du) if return_du else (dx, dw, db)


def dwconv7x7_fwd(x, wt49, bias, B, H, W, Cc):
    """x: [B*H*W, C]; wt49: fp32 [49, C] (transposed depthwise weight)."""
    y = torch.empty_like(x)
    _chk(lib().segf_dwconv7x7_fwd(dt_of(x), B, H, W, Cc, _ptr(x), _ptr(wt49), _ptr(bias), _ptr(y), _stream()),
         'segf_dwconv7x7_fwd')
    return y


def dwconv7x7_bwd(x, wt49, dy, B, H, W, Cc, need_dx=True, need_db=True):
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty((Cc, 49), dtype=torch.float32, device=x.device)
    db = torch.empty(Cc, dtype=torch.float32, device=x.device) if need_db else None
    ws = _f32(lib().segf_dwconv7x7_bwd_ws(B, H, W, Cc), x.device)
    _chk(lib().segf_dwconv7x7_bwd(dt_of(x), B, H, W, Cc, _ptr(x), _ptr(wt49), _ptr(dy), _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws),
                                  _stream()), 'segf_dwconv7x7_bwd')
    return dx, dw, db


def conv3x3(mode, x, w, B, H, W, Cin, Cout, out=None, out_dtype=None, bias=None, split_k=1):
    """Implicit-GEMM 3x3 convolution (bf16).  mode 0: y = conv(x, w[Cout, 9*Cin]); mode 1: dx from (dy, wt[Cin, 9*Cout]);
    mode 2: dw[Cout, 9*Cin] fp32 from (x, dy).  x / w / out are 2-D views with unit inner stride."""
    _need_cuda(x, w)
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.stride(-1) == 1 and w.stride(-1) == 1
    P = B * H * W
    shape = {0: (P, Cout), 1: (P, Cin), 2: (Cout, 9 * Cin)}[mode]
    if out is None:
        out = torch.empty(shape, dtype=out_dtype or (torch.float32 if mode == 2 else x.dtype), device=x.device)
    if mode != 2:
        # few output tiles over a long reduction (PPM bottleneck, the small FPN levels): split-K slices of the eight-phase tile (segfac.h)
        split_k = int(lib().segf_conv3x3_fwd_splitk(mode, B, H, W, Cin, Cout)) if (bias is None and out.dtype == torch.bfloat16) else 1
    ws = _f32(split_k * shape[0] * shape[1], x.device) if split_k > 1 else None
    key = ('conv3x3', mode, P, Cin, Cout)
    _chk(_timed(key, lambda: lib().segf_conv3x3(mode, B, H, W, Cin, Cout, _ptr(x), x.stride(0), _ptr(w), w.stride(0), _ptr(out),
                                                dt_of(out), out.stride(0), _ptr(bias), split_k, _ptr(ws), _stream())),
         'segf_conv3x3')
    return out


def conv3x3_dil_live_taps(H, W, dilation):
    """The taps ty * 3 + tx of a 3x3 kernel at this dilation that can touch an H x W map (no GPU needed)."""
    taps = (C.c_int * 9)()
    n = lib().segf_conv3x3_dil_live_taps(H, W, dilation, C.cast(taps, C.c_void_p))
    if n < 0:
        raise ValueError(f'conv3x3_dil_live_taps: bad geometry H={H} W={W} dilation={dilation}')
    return [int(taps[i]) for i in range(n)]


def conv3x3_dil_supported(dtype, mode, B, H, W, Cin, Cout, dilation):
    dt = BF16 if dtype == torch.bfloat16 else (F32 if dtype == torch.float32 else -1)
    return bool(lib().segf_conv3x3_dil_supported(dt, mode, B, H, W, Cin, Cout, dilation))


def pick_splitk_conv3x3_dil(B, H, W, Cin, Cout, dilation):
    return lib().segf_conv3x3_dil_pick_splitk(B, H, W, Cin, Cout, dilation)


def conv3x3_dil(mode, x, w, B, H, W, Cin, Cout, dilation, out=None):
    """Dilated 3x3 convolution (padding = dilation) as an implicit GEMM over the live taps, bf16 or fp32.  mode 0: y = conv(x,
    w[Cout, 9*Cin]); mode 1: dx from (dy, wt[Cin, 9*Cout]); mode 2: dw[Cout, 9*Cin] fp32 from (x, dy).  x / w / out are 2-D views with
    unit inner stride (column slices of wider buffers are fine)."""
    _need_cuda(x, w)
    assert x.dtype == w.dtype and x.stride(-1) == 1 and w.stride(-1) == 1
    P = B * H * W
    shape = {0: (P, Cout), 1: (P, Cin), 2: (Cout, 9 * Cin)}[mode]
    if out is None:
        out = torch.empty(shape, dtype=torch.float32 if mode == 2 else x.dtype, device=x.device)
    split_k = int(lib().segf_conv3x3_dil_pick_splitk(B, H, W, Cin, Cout, dilation)) if mode == 2 else 1
    ws = _f32(split_k * shape[0] * shape[1], x.device) if split_k > 1 else None
    key = ('conv3x3_dil', mode, P, Cin, Cout, dilation)
    _chk(_timed(key, lambda: lib().segf_conv3x3_dil(dt_of(x), mode, B, H, W, Cin, Cout, dilation, _ptr(x), x.stride(0), _ptr(w), w.stride(0),
                                                    _ptr(out), out.stride(0), split_k, _ptr(ws), _stream())), 'segf_conv3x3_dil')
    return out


def mul_scale(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """y[r, c] = x[r, c] * scale[r, c]; scale fp32, contiguous (elementwise dropout and its backward)."""
    _need_cuda(x, scale)
    rows, cols = x.shape
    assert scale.dtype == torch.float32 and scale.is_contiguous() and scale.numel() == rows * cols and x.stride(1) == 1
    y = torch.empty((rows, cols), dtype=x.dtype, device=x.device)
    _chk(lib().segf_mul_scale(dt_of(x), _ptr(x), x.stride(0), _ptr(scale), _ptr(y), cols, rows, cols, _stream()), 'segf_mul_scale')
    return y


def gelu_fwd(u):
    y = torch.empty_like(u)
    _chk(lib().segf_gelu(dt_of(u), 0, _ptr(u), None, _ptr(y), u.numel(), _stream()), 'segf_gelu')
    return y


def gelu_bwd(u, dy):
    du = torch.empty_like(u)
    _chk(lib().segf_gelu(dt_of(u), 1, _ptr(u), _ptr(dy), _ptr(du), u.numel(), _stream()), 'segf_gelu')
    return du


def rowdot(a, b, extra_a=None, extra_b=None):
    """out[r] = sum_c a[r, c] * b[r, c] (+ extra_a[r] * extra_b[r]); fp32 2-D inputs."""
    rows, cols = a.shape
    out = torch.empty(rows, dtype=torch.float32, device=a.device)
    _chk(lib().segf_rowdot(_ptr(a), a.stride(0), _ptr(b), b.stride(0), _ptr(extra_a), _ptr(extra_b), _ptr(out), rows, cols,
                           _stream()), 'segf_rowdot')
    return out


def adaptive_avgpool(x, B, H, W, Cc, S, bwd=False):
    """bwd=False: x [B*H*W, C] -> [B*S*S, C];  bwd=True: x = dout [B*S*S, C] -> din [B*H*W, C]."""
    out = torch.empty(((B * H * W) if bwd else (B * S * S), Cc), dtype=x.dtype, device=x.device)
    _chk(lib().segf_adaptive_avgpool(dt_of(x), int(bwd), B, H, W, Cc, S, _ptr(x), _ptr(out), _stream()), 'segf_adaptive_avgpool')
    return out


def im2col(x, dtype, in_nchw_f32, B, H, W, Cin, kh, kw, stride, pad, Ho, Wo, ldcol):
    _need_cuda(x)
    col = torch.empty((B * Ho * Wo, ldcol), dtype=dtype, device=x.device)
    _chk(lib().segf_im2col(BF16 if dtype == torch.bfloat16 else F32, int(in_nchw_f32), B, H, W, Cin, kh, kw, stride, pad,
                           Ho, Wo, _ptr(x), _ptr(col), ldcol, _stream()), 'segf_im2col')
    return col


def col2im(dcol, B, H, W, Cin, kh, kw, stride, pad, Ho, Wo):
    dx = torch.empty((B * H * W, Cin), dtype=dcol.dtype, device=dcol.device)
    _chk(lib().segf_col2im(dt_of(dcol), B, H, W, Cin, kh, kw, stride, pad, Ho, Wo, _ptr(dcol), dcol.stride(0), _ptr(dx),
                           _stream()), 'segf_col2im')
    return dx


def bilinear_fwd(x, B, h, w, Cc, H, W, out, align_corners=False):
    """x: [B*h*w, >=C] view; out: [B*H*W, >=C] view (may be a column slice of a concat buffer)."""
    _chk(lib().segf_bilinear_fwd(dt_of(x), B, h, w, Cc, _ptr(x), x.stride(0), H, W, _ptr(out), out.stride(0),
                                 int(align_corners), _stream()), 'segf_bilinear_fwd')
    return out


def argmax_rows(x, Cc):
    """int64 [rows]: arg max over the first Cc columns of x [rows, >= Cc] (lowest index on ties)."""
    _need_cuda(x)
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    _chk(lib().segf_argmax_rows(dt_of(x), x.shape[0], Cc, _ptr(x), x.stride(0), _ptr(out), _stream()), 'segf_argmax_rows')
    return out


def bilinear_bwd(dout, B, h, w, Cc, H, W, align_corners=False, ld_in=None):
    ld_in = Cc if ld_in is None else ld_in
    din = torch.empty((B * h * w, ld_in), dtype=dout.dtype, device=dout.device) if ld_in == Cc else zeros((B * h * w, ld_in), dout.dtype, dout.device)
    _chk(lib().segf_bilinear_bwd(dt_of(dout), B, h, w, Cc, _ptr(din), ld_in, H, W, _ptr(dout), dout.stride(0),
                                 int(align_corners), _stream()), 'segf_bilinear_bwd')
    return din


def nearest_up(x, B, h, w, Cc, H, W, base=None, bwd=False):
    """bwd=False: x [B*h*w, C] -> [B*H*W, C], nearest source per destination (integer factors or ATen's floorf(dst * in / out) for
    any other pair of sizes) (+ base); bwd=True: x = dout [B*H*W, C] -> sums over each source's destinations [B*h*w, C]."""
    _need_cuda(x, base)
    assert x.is_contiguous() and (base is None or base.is_contiguous())
    out = torch.empty(((B * h * w) if bwd else (B * H * W), Cc), dtype=x.dtype, device=x.device)
    _chk(lib().segf_nearest_up(dt_of(x), int(bwd), B, h, w, Cc, H, W, _ptr(x), _ptr(base), _ptr(out), _stream()), 'segf_nearest_up')
    return out


def input_train(samples, B, H, W, mean3, std3, label_lut, out_img=None, out_lbl=None):
    """segf_input_train: `samples` = uint8 device tensor holding B packed InputSample records (their image / label pointers must
    stay alive until the stream has run the kernels) -> (fp32 [B, 3, H, W], int64 [B, H, W])."""
    _need_cuda(samples, mean3, std3, label_lut)
    assert samples.dtype == torch.uint8 and samples.numel() == B * C.sizeof(InputSample)
    assert mean3.dtype == torch.float32 and std3.dtype == torch.float32 and mean3.numel() == 3 and std3.numel() == 3
    assert label_lut is None or (label_lut.dtype == torch.int64 and label_lut.numel() == 256)
    dev = samples.device
    if out_img is None:
        out_img = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    if out_lbl is None:
        out_lbl = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    assert out_img.is_contiguous() and out_lbl.is_contiguous() and out_img.numel() == B * 3 * H * W and out_lbl.numel() == B * H * W
    lsum = torch.empty(max(B, 2), dtype=torch.int64, device=dev)
    _chk(lib().segf_input_train(_ptr(samples), B, H, W, _ptr(lsum), _ptr(mean3), _ptr(std3), _ptr(label_lut), _ptr(out_img),
                                _ptr(out_lbl), _stream()), 'segf_input_train')
    return out_img, out_lbl


def resample_ksize(in_size, out_size):
    """Taps per output pixel of Pillow's bilinear resample from `in_size` to `out_size` (csrc/input.hip resample_ksize)."""
    return int(math.ceil(max(float(in_size) / float(out_size), 1.0))) * 2 + 1


def _chk_arg(rc, name):
    """As _chk, but the host-side refusal of an argument (SEGF_ERR_SHAPE, nothing launched) is a ValueError."""
    if rc == ERR_SHAPE:
        raise ValueError(f'{name} refused its arguments (SEGF_ERR_SHAPE); nothing was launched')
    _chk(rc, name)


def input_train_scaled(samples, B, H, W, kmax, mean3, std3, label_lut, out_img=None, out_lbl=None, ws=None):
    """segf_input_train_scaled: `samples` = a HOST ctypes array of B InputScaledSample records (the library checks their values, then
    uploads them itself; their image / label pointers must stay alive until the stream has run the kernels)
    -> (fp32 [B, 3, H, W], int64 [B, H, W]).  ``ws``: a uint8 device tensor of segf_input_train_scaled_ws(B, H, W, kmax) bytes
    (default: allocated here).  ValueError when the library refuses an argument."""
    _need_cuda(mean3, std3, label_lut, out_img, out_lbl, ws)
    assert isinstance(samples, C.Array) and samples._type_ is InputScaledSample and len(samples) == B
    assert mean3.dtype == torch.float32 and std3.dtype == torch.float32 and mean3.numel() == 3 and std3.numel() == 3
    assert label_lut is None or (label_lut.dtype == torch.int64 and label_lut.numel() == 256)
    dev = mean3.device
    if out_img is None:
        out_img = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    if out_lbl is None:
        out_lbl = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    assert out_img.is_contiguous() and out_lbl.is_contiguous() and out_img.numel() == B * 3 * H * W and out_lbl.numel() == B * H * W
    assert out_img.dtype == torch.float32 and out_lbl.dtype == torch.int64
    need = int(lib().segf_input_train_scaled_ws(B, H, W, kmax))
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= need
    _chk_arg(lib().segf_input_train_scaled(C.cast(samples, C.c_void_p), B, H, W, kmax, _ptr(ws), _ptr(mean3), _ptr(std3),
                                           _ptr(label_lut), _ptr(out_img), _ptr(out_lbl), _stream()), 'segf_input_train_scaled')
    return out_img, out_lbl


def input_crop_select(samples, cand, B, K, H, W, max_ratio, label_lut, ignore_class, chosen=None):
    """segf_input_crop_select: the class-balanced choice among K candidate windows per sample (the rule: include/segfac.h).
    `samples` as for `input_train` (top / left of the device records are rewritten in place), `cand` = int32 device tensor
    [B, K, 2] of non-negative (top, left) -> `chosen`, int32 [B] on the device (nothing is read back).  ValueError when the library
    refuses an argument."""
    _need_cuda(samples, cand, label_lut, chosen)
    assert samples.dtype == torch.uint8 and samples.numel() == B * C.sizeof(InputSample)
    assert cand.dtype == torch.int32 and cand.is_contiguous() and cand.numel() == B * K * 2
    assert label_lut is None or (label_lut.dtype == torch.int64 and label_lut.numel() == 256)
    if chosen is None:
        chosen = torch.empty(B, dtype=torch.int32, device=samples.device)
    assert chosen.dtype == torch.int32 and chosen.is_contiguous() and chosen.numel() == B
    _chk_arg(lib().segf_input_crop_select(_ptr(samples), _ptr(cand), B, K, H, W, float(max_ratio), _ptr(label_lut), int(ignore_class),
                                          _ptr(chosen), _stream()), 'segf_input_crop_select')
    return chosen


def input_train_scaled_select(samples, cand, B, K, H, W, kmax, max_ratio, ignore_class, mean3, std3, label_lut, out_img=None,
                              out_lbl=None, ws=None, chosen=None):
    """segf_input_train_scaled_select: `input_train_scaled` with the class-balanced choice among K candidate windows per sample in
    front (the rule: include/segfac.h).  `cand` = a HOST ctypes c_int32 array of B * K * 2 values, (top, left) in resized
    coordinates -> (fp32 [B, 3, H, W], int64 [B, H, W], chosen int32 [B] on the device).  ``ws``: a uint8 device tensor of
    segf_input_train_scaled_select_ws(B, H, W, kmax, K) bytes (default: allocated here)."""
    _need_cuda(mean3, std3, label_lut, out_img, out_lbl, ws, chosen)
    assert isinstance(samples, C.Array) and samples._type_ is InputScaledSample and len(samples) == B
    assert isinstance(cand, C.Array) and cand._type_ is C.c_int32 and len(cand) == B * K * 2
    assert mean3.dtype == torch.float32 and std3.dtype == torch.float32 and mean3.numel() == 3 and std3.numel() == 3
    assert label_lut is None or (label_lut.dtype == torch.int64 and label_lut.numel() == 256)
    dev = mean3.device
    if out_img is None:
        out_img = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    if out_lbl is None:
        out_lbl = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    if chosen is None:
        chosen = torch.empty(B, dtype=torch.int32, device=dev)
    assert out_img.is_contiguous() and out_lbl.is_contiguous() and out_img.numel() == B * 3 * H * W and out_lbl.numel() == B * H * W
    assert out_img.dtype == torch.float32 and out_lbl.dtype == torch.int64
    assert chosen.dtype == torch.int32 and chosen.is_contiguous() and chosen.numel() == B
    need = int(lib().segf_input_train_scaled_select_ws(B, H, W, kmax, K))
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= need
    _chk_arg(lib().segf_input_train_scaled_select(C.cast(samples, C.c_void_p), C.cast(cand, C.c_void_p), K, float(max_ratio),
                                                  int(ignore_class), _ptr(chosen), B, H, W, kmax, _ptr(ws), _ptr(mean3), _ptr(std3),
                                                  _ptr(label_lut), _ptr(out_img), _ptr(out_lbl), _stream()),
             'segf_input_train_scaled_select')
    return out_img, out_lbl, chosen


def input_val(img, lbl, out_h, out_w, mean3, std3, label_lut):
    """segf_input_val: img uint8 [h, w, 3], lbl uint8 [h, w] (device) -> (fp32 [3, out_h, out_w], int64 [out_h, out_w])."""
    _need_cuda(img, lbl, mean3, std3, label_lut)
    assert img.dtype == torch.uint8 and lbl.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3 and img.stride(2) == 1 \
        and img.stride(1) == 3 and lbl.stride(1) == 1 and lbl.shape == img.shape[:2]
    assert label_lut is None or (label_lut.dtype == torch.int64 and label_lut.numel() == 256)
    h, w = int(img.shape[0]), int(img.shape[1])
    ws = torch.empty(int(lib().segf_input_val_ws(h, w, out_h, out_w)) + 16, dtype=torch.uint8, device=img.device)
    out_img = torch.empty((3, out_h, out_w), dtype=torch.float32, device=img.device)
    out_lbl = torch.empty((out_h, out_w), dtype=torch.int64, device=img.device)
    _chk(lib().segf_input_val(_ptr(img), img.stride(0), _ptr(lbl), lbl.stride(0), h, w, out_h, out_w, _ptr(ws), _ptr(mean3),
                              _ptr(std3), _ptr(label_lut), _ptr(out_img), _ptr(out_lbl), _stream()), 'segf_input_val')
    return out_img, out_lbl


def infer_preprocess(img, out_h, out_w, mean3, std3):
    """segf_infer_preprocess: uint8 [3, h, w] (device) -> fp32 [1, 3, out_h, out_w]: torchvision-0.15 tensor resize + / 255 + normalise."""
    _need_cuda(img, mean3, std3)
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[0] == 3 and img.is_contiguous()
    out = torch.empty((1, 3, out_h, out_w), dtype=torch.float32, device=img.device)
    _chk(lib().segf_infer_preprocess(_ptr(img), int(img.shape[1]), int(img.shape[2]), out_h, out_w, _ptr(mean3), _ptr(std3), _ptr(out),
                                     _stream()), 'segf_infer_preprocess')
    return out


def bilinear_bwd_248(dout, B, H, W, Cc):
    """(d2, d4, d8): transposed x2 / x4 / x8 bilinear resizes of dout [B*H*W, >= C] in one pass (segf_bilinear_bwd_248)."""
    _need_cuda(dout)
    outs = [torch.empty((B * (H // r) * (W // r), Cc), dtype=dout.dtype, device=dout.device) for r in (2, 4, 8)]
    _chk(lib().segf_bilinear_bwd_248(dt_of(dout), B, H, W, Cc, _ptr(dout), dout.stride(0), _ptr(outs[0]), _ptr(outs[1]),
                                     _ptr(outs[2]), _stream()), 'segf_bilinear_bwd_248')
    return outs


def upsample_add(base, srcs, B, H, W, Cc, align_corners=False):
    """out = base + sum_k bilinear_up(src_k); srcs = [(tokens [B*h*w, C], h, w), ...] (at most 3)."""
    out = torch.empty((B * H * W, Cc), dtype=base.dtype, device=base.device)
    a = []
    for k in range(3):
        if k < len(srcs):
            t, h, w = srcs[k]
            a += [_ptr(t), h, w, t.stride(0)]
        else:
            a += [None, 0, 0, 0]
    _chk(lib().segf_upsample_add(dt_of(base), B, H, W, Cc, _ptr(base), base.stride(0), len(srcs), *a, _ptr(out), Cc,
                                 int(align_corners), _stream()), 'segf_upsample_add')
    return out


def upsample_add_stats(base, srcs, B, H, W, Cc):
    """upsample_add that also returns sums fp32 [2, C] = per-channel (sum, sum of squares) of the stored result (the BatchNorm
    statistics of the consumer); None for the sums when the geometry is not the fused 1/2-1/4-1/8 case."""
    out = torch.empty((B * H * W, Cc), dtype=base.dtype, device=base.device)
    a = []
    for k in range(3):
        if k < len(srcs):
            t, h, w = srcs[k]
            a += [_ptr(t), h, w, t.stride(0)]
        else:
            a += [None, 0, 0, 0]
    sums = torch.empty((2, Cc), dtype=torch.float32, device=base.device)
    ws = _f32(max(1, lib().segf_upsample_add_stats_ws(B, H, W, Cc)), base.device)
    rc = lib().segf_upsample_add_stats(dt_of(base), B, H, W, Cc, _ptr(base), base.stride(0), len(srcs), *a, _ptr(out), Cc, 0,
                                       _ptr(sums), _ptr(ws), _stream())
    if rc == ERR_SHAPE:
        return upsample_add(base, srcs, B, H, W, Cc), None
    _chk(rc, 'segf_upsample_add_stats')
    return out, sums


def fuse_map_248_supported(dtype, B, H, W, Cc, C1):
    return dtype == torch.bfloat16 and bool(lib().segf_fuse_map_248_supported(BF16, B, H, W, Cc, C1))


def fuse_map_248(x1, g1, t2, t3, t4, B, H, W, with_sums=True):
    """out [B*H*W, C] = x1 g1^T + bilinear(t2) + bilinear(t3) + bilinear(t4) (1/2, 1/4, 1/8 maps, align_corners=False) and, when
    asked, sums fp32 [2, C] = per-channel (sum, sum of squares) of the result: the folded SegFormerHead's stride-4 map in one launch."""
    _need_cuda(x1, g1, t2, t3, t4)
    Cc, C1 = g1.shape
    out = torch.empty((B * H * W, Cc), dtype=torch.bfloat16, device=x1.device)
    sums = torch.empty((2, Cc), dtype=torch.float32, device=x1.device) if with_sums else None
    ws = _f32(max(1, lib().segf_fuse_map_248_ws(B, H, W, Cc)), x1.device) if with_sums else None
    _chk(lib().segf_fuse_map_248(B, H, W, Cc, C1, _ptr(x1), x1.stride(0), _ptr(g1), g1.stride(0), _ptr(t2), t2.stride(0),
                                 _ptr(t3), t3.stride(0), _ptr(t4), t4.stride(0), _ptr(out), Cc,
                                 _ptr(sums) if with_sums else None, _ptr(ws) if with_sums else None, _stream()), 'segf_fuse_map_248')
    return out, sums


def bn_stats_from_sums(sums, rows, running_mean, running_var, momentum, eps):
    Cc = sums.shape[1]
    mean = torch.empty(Cc, dtype=torch.float32, device=sums.device)
    rstd = torch.empty(Cc, dtype=torch.float32, device=sums.device)
    _chk(lib().segf_bn_stats_from_sums(_ptr(sums), rows, Cc, _ptr(mean), _ptr(rstd), _ptr(running_mean), _ptr(running_var),
                                       momentum, eps, _stream()), 'segf_bn_stats_from_sums')
    return mean, rstd


def bilinear_to_nchw_f32(x, B, h, w, Cc, H, W):
    out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=x.device)
    _chk(lib().segf_bilinear_to_nchw_f32(dt_of(x), B, h, w, Cc, _ptr(x), x.stride(0), H, W, _ptr(out), _stream()),
         'segf_bilinear_to_nchw_f32')
    return out


# ---- loss / metrics ------------------------------------------------------------------------------------
def ce_dice_fwd(logits, B, Cc, h, w, H, W, target, ignore_index, class_weight, dice, want_lse=False):
    """(loss[3], stats) or, with want_lse, (loss[3], stats, lse): lse = the per-pixel log-sum buffer for ce_dice_bwd of the
    same logits (None when this configuration does not produce one)."""
    stats = _f32(lib().segf_ce_dice_stats_floats(B, Cc), logits.device)
    loss = torch.empty(3, dtype=torch.float32, device=logits.device)
    lse = None
    if want_lse:
        n = lib().segf_ce_dice_lse_floats(dt_of(logits), B, Cc, h, w, H, W, _ptr(logits), logits.stride(0))
        lse = torch.empty(n, dtype=torch.float32, device=logits.device) if n else None
    _chk(lib().segf_ce_dice_fwd(dt_of(logits), B, Cc, h, w, H, W, _ptr(logits), logits.stride(0), _ptr(target),
                                int(ignore_index), _ptr(class_weight), int(dice), _ptr(stats), _ptr(loss), _ptr(lse), _stream()),
         'segf_ce_dice_fwd')
    return (loss, stats, lse) if want_lse else (loss, stats)


def ce_dice_bwd(logits, B, Cc, h, w, H, W, target, ignore_index, class_weight, dice, stats, grad_out, lse=None):
    """d loss / d (low-res logits), same row stride as `logits` (pad columns zeroed).  lse: ce_dice_fwd(want_lse=True)'s."""
    ld = logits.stride(0)
    dlow = torch.empty((B * h * w, ld), dtype=logits.dtype, device=logits.device)
    dt = dt_of(logits)
    nws = lib().segf_ce_dice_bwd_ws(dt, B, Cc, h, w, H, W)
    ws = _f32(nws, logits.device) if nws else None
    _chk(_timed(('ce_dice_bwd', B, Cc, h, w, H, W), lambda: lib().segf_ce_dice_bwd(
        dt, B, Cc, h, w, H, W, _ptr(logits), ld, _ptr(target), int(ignore_index), _ptr(class_weight), int(dice), _ptr(stats),
        _ptr(grad_out), _ptr(dlow), ld, _ptr(ws), _ptr(lse), _stream())), 'segf_ce_dice_bwd')
    return dlow


PIXEL_OHEM, PIXEL_FOCAL = 0, 1          # mode of segf_pixel_loss_*


def pixel_loss_supported(dtype, mode, B, Cc, h, w, H, W):
    dt = {torch.float32: F32, torch.bfloat16: BF16}.get(dtype, -1)
    return bool(lib().segf_pixel_loss_supported(dt, int(mode), B, Cc, h, w, H, W))


def pixel_loss_fwd(logits, B, Cc, h, w, H, W, target, ignore_index, class_weight, mode, p0, p1, size_average):
    """(loss[1], ce_map [B, H, W] fp32, state int32): state[:8] is the layout documented in include/segfac.h (kappa's fp32 bits at 6)."""
    n = lib().segf_pixel_loss_state_words(B)
    if n <= 0:
        raise RuntimeError(f'segf_pixel_loss_state_words: unsupported batch size {B}')
    state = torch.empty(n, dtype=torch.int32, device=logits.device)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    ce_map = torch.empty((B, H, W), dtype=torch.float32, device=logits.device)
    _chk(lib().segf_pixel_loss_fwd(dt_of(logits), int(mode), B, Cc, h, w, H, W, _ptr(logits), logits.stride(0), _ptr(target),
                                   int(ignore_index), _ptr(class_weight), float(p0), float(p1), int(size_average), _ptr(ce_map),
                                   _ptr(state), _ptr(loss), _stream()), 'segf_pixel_loss_fwd')
    return loss, ce_map, state


def pixel_loss_bwd(logits, B, Cc, h, w, H, W, target, ignore_index, class_weight, mode, p0, p1, size_average, ce_map, state,
                   grad_out):
    """d loss / d (low-res logits), same row stride as `logits` (pad columns zeroed), from pixel_loss_fwd's ce_map and state."""
    ld = logits.stride(0)
    dlow = torch.empty((B * h * w, ld), dtype=logits.dtype, device=logits.device)
    dt = dt_of(logits)
    nws = lib().segf_pixel_loss_bwd_ws(dt, B, Cc, h, w, H, W)
    ws = _f32(nws, logits.device) if nws else None
    _chk(lib().segf_pixel_loss_bwd(dt, int(mode), B, Cc, h, w, H, W, _ptr(logits), ld, _ptr(target), int(ignore_index),
                                   _ptr(class_weight), float(p0), float(p1), int(size_average), _ptr(ce_map), _ptr(state),
                                   _ptr(grad_out), _ptr(dlow), ld, _ptr(ws), _stream()), 'segf_pixel_loss_bwd')
    return dlow


def argmax_confmat(logits, B, Cc, h, w, H, W, target, ignore_label, mat, hist, flag, pred_out=None):
    _chk(lib().segf_argmax_confmat(dt_of(logits), B, Cc, h, w, H, W, _ptr(logits), logits.stride(0), _ptr(target),
                                   int(ignore_label), _ptr(mat), _ptr(hist), _ptr(flag), _ptr(pred_out), _stream()),
         'segf_argmax_confmat')


MSF_MAX_MAPS = 16          # SEGF_MSF_MAX_MAPS of include/segfac.h


def msf_argmax_confmat(maps, flips, B, Cc, H, W, target, ignore_label, mat, hist, flag, pred_out=None, prob_out=None):
    """segf_msf_argmax_confmat: multi-scale + flip evaluation in one kernel.  maps: TokenMaps (or (rows, h, w) tuples; rows =
    [B*h*w, >= Cc] with unit inner stride, all one dtype); flips: one flag per map (the map belongs to the mirrored image).  Per pixel of
    the (H, W) output: bilinear sample of every map, softmax, sum in list order, arg max -> mat / hist / flag as argmax_confmat
    (target None: no counting), pred_out int64 [B, H, W], prob_out fp32 [B*H*W, >= Cc] = the summed probabilities.  The descriptors go
    by value through host arrays: nothing is uploaded, so the call can be captured."""
    n = len(maps)
    if len(flips) != n:
        raise ValueError(f'msf_argmax_confmat: {n} maps but {len(flips)} flip flags')
    rows, hw = [], []
    for m in maps:
        data, h, w = (m.data, m.H, m.W) if hasattr(m, 'data') else m
        _need_cuda(data)
        if (data.dtype != (rows[0].dtype if rows else data.dtype) or data.ndim != 2 or data.stride(1) != 1 or data.shape[0] != B * h * w
                or data.shape[1] < Cc):
            raise ValueError('msf_argmax_confmat: maps must share one dtype and be [B*h*w, >=C] rows with unit inner stride')
        rows.append(data)
        hw += [int(h), int(w)]
    _need_cuda(target, mat, hist, flag, pred_out, prob_out)
    if target is not None:
        assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == B * H * W
        assert all(t.dtype == torch.int64 and t.is_contiguous() and t.numel() == Cc * Cc for t in (mat, hist)) and flag.dtype == torch.int32
    assert pred_out is None or (pred_out.dtype == torch.int64 and pred_out.is_contiguous() and pred_out.numel() == B * H * W)
    assert prob_out is None or (prob_out.dtype == torch.float32 and prob_out.ndim == 2 and prob_out.stride(1) == 1
                                and prob_out.shape[0] == B * H * W and prob_out.shape[1] >= Cc)
    ptrs = (C.c_void_p * max(n, 1))(*[r.data_ptr() for r in rows])
    c_hw = (C.c_int * max(2 * n, 1))(*hw)
    c_ld = (C.c_int64 * max(n, 1))(*[r.stride(0) for r in rows])
    c_fl = (C.c_int * max(n, 1))(*[1 if f else 0 for f in flips])
    _chk(lib().segf_msf_argmax_confmat(dt_of(rows[0]) if rows else F32, B, Cc, n, ptrs, c_hw, c_ld, c_fl, H, W, _ptr(target),
                                       int(ignore_label), _ptr(mat), _ptr(hist), _ptr(flag), _ptr(pred_out), _ptr(prob_out),
                                       prob_out.stride(0) if prob_out is not None else 0, _stream()), 'segf_msf_argmax_confmat')


def hw_pair(v, name='size'):
    """(rows, columns) of an int, a 1-list or a pair: crop / stride of the sliding-window calls."""
    v = tuple(v) if isinstance(v, (tuple, list)) else (v,)
    if len(v) not in (1, 2):
        raise ValueError(f'{name}: expected H or (H, W), got {v!r}')
    return int(v[0]), int(v[-1])


def slide_grid(H, W, crop, stride):
    """segf_slide_grid: (ny, nx) of the sliding-window grid over an H x W image -- n = max(L - crop + stride - 1, 0) // stride + 1
    per axis, window i at min(i stride, L - crop).  crop / stride: an int or (rows, columns).  ValueError for a grid the library
    refuses (1 <= stride <= crop <= image violated)."""
    (ch, cw), (sh, sw) = hw_pair(crop, 'crop'), hw_pair(stride, 'stride')
    ny, nx = _i(), _i()
    if lib().segf_slide_grid(int(H), int(W), ch, cw, sh, sw, C.byref(ny), C.byref(nx)) != 0:
        raise ValueError(f'slide_grid: 1 <= stride <= crop <= image violated (image {H} x {W}, crop {ch} x {cw}, stride {sh} x {sw})')
    return ny.value, nx.value


def slide_argmax_confmat(windows, B, Cc, H, W, crop, stride, target, ignore_label, mat, hist, flag, pred_out=None, mean_out=None):
    """segf_slide_argmax_confmat: sliding-window evaluation in one kernel.  windows: a TokenMap (or a (rows, h, w) tuple) holding the
    head outputs of all windows of the batch, rows = [B*ny*nx*h*w, >= Cc] with unit inner stride, image-major, then window order
    (i nx + j; slide_grid gives ny, nx).  Per pixel of the (H, W) output: bilinear sample of every covering window's map at the local
    pixel, summed in window order, divided by the cover count, arg max -> mat / hist / flag as argmax_confmat (target None: no
    counting), pred_out int64 [B, H, W], mean_out fp32 [B*H*W, >= Cc] = the mean logits.  Nothing is uploaded: the call can be
    captured."""
    (ch, cw), (sh, sw) = hw_pair(crop, 'crop'), hw_pair(stride, 'stride')
    ny, nx = slide_grid(H, W, (ch, cw), (sh, sw))
    data, h, w = (windows.data, windows.H, windows.W) if hasattr(windows, 'data') else windows
    h, w = int(h), int(w)
    _need_cuda(data, target, mat, hist, flag, pred_out, mean_out)
    if data.ndim != 2 or data.stride(1) != 1 or data.shape[0] != B * ny * nx * h * w or data.shape[1] < Cc:
        raise ValueError(f'slide_argmax_confmat: windows must be [B*ny*nx*h*w, >=C] rows with unit inner stride '
                         f'(B {B}, grid {ny} x {nx}, map {h} x {w}, C {Cc}; got {tuple(data.shape)}, strides {tuple(data.stride())})')
    if hasattr(windows, 'B') and windows.B != B * ny * nx:
        raise ValueError(f'slide_argmax_confmat: {windows.B} window maps, expected B*ny*nx = {B * ny * nx}')
    if target is not None:
        assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == B * H * W
        assert all(t.dtype == torch.int64 and t.is_contiguous() and t.numel() == Cc * Cc for t in (mat, hist)) and flag.dtype == torch.int32
    assert pred_out is None or (pred_out.dtype == torch.int64 and pred_out.is_contiguous() and pred_out.numel() == B * H * W)
    assert mean_out is None or (mean_out.dtype == torch.float32 and mean_out.ndim == 2 and mean_out.stride(1) == 1
                                and mean_out.shape[0] == B * H * W and mean_out.shape[1] >= Cc)
    _chk(lib().segf_slide_argmax_confmat(dt_of(data), B, Cc, H, W, ch, cw, sh, sw, h, w, _ptr(data), data.stride(0), _ptr(target),
                                         int(ignore_label), _ptr(mat), _ptr(hist), _ptr(flag), _ptr(pred_out), _ptr(mean_out),
                                         mean_out.stride(0) if mean_out is not None else 0, _stream()), 'segf_slide_argmax_confmat')


def msf_slide_argmax_confmat(window_sets, flips, B, Cc, H, W, target, ignore_label, mat, hist, flag, pred_out=None, prob_out=None):
    """segf_msf_slide_argmax_confmat: multi-scale + flip sliding-window evaluation in one kernel.  window_sets: one entry per
    (scale, flip) pair, `(windows, (Hs, Ws), crop, stride)` -- windows a TokenMap (or a (rows, h, w) tuple) holding the head outputs
    of all windows of the batch cut from the (Hs, Ws) scaled image, rows = [B*ny*nx*h*w, >= Cc] with unit inner stride, image-major,
    then window order (slide_grid(Hs, Ws, crop, stride) gives ny, nx; crop / stride already clamped as engine.slide_windows does), all
    sets one dtype; flips: one flag per set (the set belongs to the mirrored image).  Per pixel of the (H, W) output and per set: the
    window mean of slide_argmax_confmat at the taps of the resize from (Hs, Ws), softmax, sum in list order, arg max -> mat / hist /
    flag as argmax_confmat (target None: no counting), pred_out int64 [B, H, W], prob_out fp32 [B*H*W, >= Cc] = the summed
    probabilities.  The descriptors go by value through host arrays: nothing is uploaded, so the call can be captured."""
    n = len(window_sets)
    if len(flips) != n:
        raise ValueError(f'msf_slide_argmax_confmat: {n} window sets but {len(flips)} flip flags')
    rows, geom = [], []
    for k, (windows, (Hs, Ws), crop, stride) in enumerate(window_sets):
        (ch, cw), (sh, sw) = hw_pair(crop, 'crop'), hw_pair(stride, 'stride')
        ny, nx = slide_grid(Hs, Ws, (ch, cw), (sh, sw))
        data, h, w = (windows.data, windows.H, windows.W) if hasattr(windows, 'data') else windows
        h, w = int(h), int(w)
        _need_cuda(data)
        if data.ndim != 2 or data.stride(1) != 1 or data.shape[0] != B * ny * nx * h * w or data.shape[1] < Cc:
            raise ValueError(f'msf_slide_argmax_confmat: set {k} must be [B*ny*nx*h*w, >=C] rows with unit inner stride '
                             f'(B {B}, grid {ny} x {nx}, map {h} x {w}, C {Cc}; got {tuple(data.shape)}, strides {tuple(data.stride())})')
        if hasattr(windows, 'B') and windows.B != B * ny * nx:
            raise ValueError(f'msf_slide_argmax_confmat: set {k} holds {windows.B} window maps, expected B*ny*nx = {B * ny * nx}')
        if rows and data.dtype != rows[0].dtype:
            raise ValueError('msf_slide_argmax_confmat: the window sets must share one dtype')
        rows.append(data)
        geom += [int(Hs), int(Ws), ch, cw, sh, sw, h, w]
    _need_cuda(target, mat, hist, flag, pred_out, prob_out)
    if target is not None:
        assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == B * H * W
        assert all(t.dtype == torch.int64 and t.is_contiguous() and t.numel() == Cc * Cc for t in (mat, hist)) and flag.dtype == torch.int32
    assert pred_out is None or (pred_out.dtype == torch.int64 and pred_out.is_contiguous() and pred_out.numel() == B * H * W)
    assert prob_out is None or (prob_out.dtype == torch.float32 and prob_out.ndim == 2 and prob_out.stride(1) == 1
                                and prob_out.shape[0] == B * H * W and prob_out.shape[1] >= Cc)
    ptrs = (C.c_void_p * max(n, 1))(*[r.data_ptr() for r in rows])
    c_geom = (C.c_int * max(8 * n, 1))(*geom)
    c_ld = (C.c_int64 * max(n, 1))(*[r.stride(0) for r in rows])
    c_fl = (C.c_int * max(n, 1))(*[1 if f else 0 for f in flips])
    _chk(lib().segf_msf_slide_argmax_confmat(dt_of(rows[0]) if rows else F32, B, Cc, n, ptrs, c_geom, c_ld, c_fl, H, W, _ptr(target),
                                             int(ignore_label), _ptr(mat), _ptr(hist), _ptr(flag), _ptr(pred_out), _ptr(prob_out),
                                             prob_out.stride(0) if prob_out is not None else 0, _stream()),
         'segf_msf_slide_argmax_confmat')


def confmat_pairs(gt, pred, Cc, ignore_label, mat, hist, flag):
    _need_cuda(gt, pred)
    _chk(lib().segf_confmat_pairs(_ptr(gt), _ptr(pred), gt.numel(), Cc, int(ignore_label), _ptr(mat), _ptr(hist),
                                  _ptr(flag), _stream()), 'segf_confmat_pairs')


def clip_grad(grad, mode, value, ws=None):
    """segf_clip_grad on a flat fp32 gradient buffer, in place: mode 'norm' (clip_grad_norm_, L2) or 'value' (clip_grad_value_)."""
    _need_cuda(grad)
    assert grad.dtype == torch.float32 and grad.is_contiguous()
    m = {'norm': 0, 'value': 1}[mode]
    if m == 0 and ws is None:
        ws = _f32(lib().segf_clip_grad_ws(), grad.device)
    _chk(lib().segf_clip_grad(_ptr(grad), grad.numel(), m, float(value), _ptr(ws), _stream()), 'segf_clip_grad')
    return grad


def agc_adamw(param, grad, exp_avg, exp_avg_sq, unit_off, unit_len, unit_flags, lr, beta1, beta2, eps, weight_decay,
              step, clip_factor, agc_eps=1e-3, unit_step=None):
    _chk(lib().segf_agc_adamw(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(unit_off), _ptr(unit_len),
                              _ptr(unit_flags), _ptr(unit_step) if unit_step is not None else None, unit_len.numel(), lr, beta1, beta2, eps, weight_decay, step, clip_factor,
                              agc_eps, _stream()), 'segf_agc_adamw')


OPT_RULES = {'sgd': 0, 'adam': 1, 'rmsprop': 2}          # SEGF_OPT_* of include/segfac.h


def flat_optim_step(rule, param, grad, s0, s1, unit_off, unit_len, unit_flags, unit_step, lr, weight_decay, h0, h1=0.0, eps=0.0,
                    nesterov=False, clip_factor=0.0, agc_eps=1e-3):
    """segf_flat_optim_step: one SGD / Adam / RMSprop step over the flat buffers (h0, h1: momentum | beta1, beta2 | alpha, momentum);
    s0 / s1 are the rule's flat state buffers, None where it keeps none."""
    _need_cuda(param, grad, s0, s1, unit_off, unit_len, unit_flags, unit_step)
    _chk(lib().segf_flat_optim_step(OPT_RULES[rule], _ptr(param), _ptr(grad), _ptr(s0), _ptr(s1), _ptr(unit_off), _ptr(unit_len),
                                    _ptr(unit_flags), _ptr(unit_step), unit_len.numel(), lr, weight_decay, h0, h1, eps,
                                    int(bool(nesterov)), clip_factor, agc_eps, _stream()), 'segf_flat_optim_step')


OPT_MAX_GROUPS = 128          # SEGF_OPT_MAX_GROUPS of include/segfac.h


def _group_tables(group_lr, group_wd):
    """(ngroups, host float arrays) of the per-group learning rates / weight decays: the library copies them into the kernel's
    by-value argument at launch, so they are plain host memory that only has to live until the call returns."""
    n = len(group_lr)
    assert len(group_wd) == n
    return n, (_f * max(n, 1))(*group_lr), (_f * max(n, 1))(*group_wd)


def agc_adamw_groups(param, grad, exp_avg, exp_avg_sq, unit_off, unit_len, unit_flags, unit_group, group_lr, group_wd, beta1, beta2,
                     eps, step, clip_factor, agc_eps=1e-3, unit_step=None):
    """segf_agc_adamw_groups: segf_agc_adamw with the learning rate and weight decay of unit u taken from group unit_group[u]
    (device uint8 [nunits]); group_lr / group_wd are host sequences of one value per group."""
    _need_cuda(param, grad, exp_avg, exp_avg_sq, unit_off, unit_len, unit_flags, unit_group, unit_step)
    n, lrs, wds = _group_tables(group_lr, group_wd)
    _chk(lib().segf_agc_adamw_groups(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(unit_off), _ptr(unit_len),
                                     _ptr(unit_flags), _ptr(unit_step), unit_len.numel(), _ptr(unit_group), n, lrs, wds, beta1, beta2,
                                     eps, step, clip_factor, agc_eps, _stream()), 'segf_agc_adamw_groups')


def flat_optim_step_groups(rule, param, grad, s0, s1, unit_off, unit_len, unit_flags, unit_step, unit_group, group_lr, group_wd, h0,
                           h1=0.0, eps=0.0, nesterov=False, clip_factor=0.0, agc_eps=1e-3):
    """segf_flat_optim_step_groups: segf_flat_optim_step with per-group learning rate and weight decay (see agc_adamw_groups)."""
    _need_cuda(param, grad, s0, s1, unit_off, unit_len, unit_flags, unit_step, unit_group)
    n, lrs, wds = _group_tables(group_lr, group_wd)
    _chk(lib().segf_flat_optim_step_groups(OPT_RULES[rule], _ptr(param), _ptr(grad), _ptr(s0), _ptr(s1), _ptr(unit_off),
                                           _ptr(unit_len), _ptr(unit_flags), _ptr(unit_step), unit_len.numel(), _ptr(unit_group), n,
                                           lrs, wds, h0, h1, eps, int(bool(nesterov)), clip_factor, agc_eps, _stream()),
         'segf_flat_optim_step_groups')
