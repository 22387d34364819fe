"""Run the MATLAB gateway (em_model_manned_bayes_amd/matlab/emgpu_mex.c) without MATLAB: compile it together with the working mex
runtime of tests/stubs/mex_runtime.c into one shared object, and call its mexFunction through ctypes with numpy arrays.

    gw = mexrt.build(tmp_dir)
    s = gw.call("em_read", path)                       # one output
    init, cnt, E = gw.call("sample_uncor", h, ..., nlhs=3)

numpy -> mxArray: float / int -> double scalar, bool -> logical scalar, str -> char row, float64 / bool / uint8 / uint64 arrays ->
arrays of that class with the numpy shape as MATLAB dims (a 1-d array is a row), list -> 1 x k cell, object array -> cell of that
shape, dict -> 1 x 1 struct; None inside a cell is an unset cell (what cell(1, k) holds).
mxArray -> numpy: FORTRAN-ordered arrays with MATLAB's dims, so a test indexes them exactly as the .m files do (E[:cnt[i], :, i]);
char -> str, cell -> object array, struct -> dict.

Every call checks the runtime's guard words and violation record (see mex_runtime.c) and raises MexError(identifier, message) when the
gateway called mexErrMsgIdAndTxt."""
import ctypes as C
import os
import subprocess

import numpy as np

from em_model_manned_bayes_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATEWAY_SOURCE = os.path.join(ROOT, "em_model_manned_bayes_amd", "matlab", "emgpu_mex.c")
RUNTIME_SOURCE = os.path.join(ROOT, "tests", "stubs", "mex_runtime.c")

CELL, STRUCT, LOGICAL, CHAR, DOUBLE, UINT8, UINT64 = 1, 2, 3, 4, 6, 9, 13
_DTYPE = {DOUBLE: np.float64, UINT8: np.uint8, UINT64: np.uint64, LOGICAL: np.bool_, CHAR: np.uint16}
_CLASS = {np.dtype(np.float64): DOUBLE, np.dtype(np.uint8): UINT8, np.dtype(np.uint64): UINT64, np.dtype(np.bool_): LOGICAL}
MAX_OUT = 8


class MexError(RuntimeError):
    def __init__(self, identifier, message):
        super().__init__("%s: %s" % (identifier, message))
        self.identifier, self.message = identifier, message


def gateway_source():
    """The gateway's source file; EMGPU_MEX_SOURCE names another one (a mutated throwaway copy, for checking that the tests notice)."""
    return os.environ.get("EMGPU_MEX_SOURCE") or GATEWAY_SOURCE


def build(out_dir, source=None):
    """Compile gateway + runtime with gcc -std=c99 -Wall -Werror (no hipcc, no MATLAB) and load the object.  libemgpu.so is loaded FIRST,
    through the package, and the object is linked against it with an rpath to the package directory: the loader then reuses the library
    that is already mapped instead of mapping a second one (and with it a second HIP runtime)."""
    pkg = os.path.dirname(L.LIB_PATH)
    so = os.path.join(str(out_dir), "emgpu_mex_test.so")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-g", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tests", "stubs"),
                           "-I" + os.path.join(ROOT, "include"), source or gateway_source(), RUNTIME_SOURCE, "-o", so,
                           "-L" + pkg, "-lemgpu", "-lm", "-Wl,-rpath," + pkg])
    L.lib()
    return Gateway(C.CDLL(so))


class Gateway:
    def __init__(self, dll):
        self.dll = d = dll
        P, Z = C.c_void_p, C.c_size_t
        for name, res, args in (("rt_call", C.c_int, [C.c_int, C.POINTER(P), C.c_int, C.POINTER(P)]), ("rt_error_id", C.c_char_p, []),
                                ("rt_error_msg", C.c_char_p, []), ("rt_check_guards", C.c_int, []), ("rt_violation_count", C.c_int, []),
                                ("rt_violations", C.c_char_p, []), ("rt_clear_violations", None, []), ("rt_live_arrays", C.c_int, []),
                                ("rt_live_blocks", C.c_int, []), ("rt_run_at_exit", C.c_int, []), ("rt_at_exit_registrations", C.c_int, []),
                                ("rt_destroy", None, [P]), ("rt_class", C.c_int, [P]), ("rt_ndim", C.c_int, [P]), ("rt_dim", Z, [P, C.c_int]),
                                ("rt_nfields", C.c_int, [P]), ("rt_fieldname", C.c_char_p, [P, C.c_int]), ("rt_new", P, [C.c_int, C.c_int, C.POINTER(Z)]),
                                ("mxGetData", P, [P]), ("mxCreateString", P, [C.c_char_p]), ("mxCreateCellMatrix", P, [Z, Z]),
                                ("mxCreateStructMatrix", P, [Z, Z, C.c_int, C.POINTER(C.c_char_p)]), ("mxSetCell", None, [P, Z, P]),
                                ("mxGetCell", P, [P, Z]), ("mxSetField", None, [P, Z, C.c_char_p, P]), ("mxGetField", P, [P, Z, C.c_char_p])):
            f = getattr(d, name)
            f.restype, f.argtypes = res, args

    # ---- numpy -> mxArray
    def to_mx(self, v):
        d = self.dll
        if isinstance(v, str):
            return d.mxCreateString(v.encode("latin-1"))
        if isinstance(v, dict):
            names = list(v)
            arr = (C.c_char_p * max(len(names), 1))(*[k.encode() for k in names])
            s = d.mxCreateStructMatrix(1, 1, len(names), arr)
            for k in names:
                if v[k] is not None:
                    d.mxSetField(s, 0, k.encode(), self.to_mx(v[k]))
            return s
        if isinstance(v, (list, tuple)):
            o = np.empty((1, len(v)), dtype=object)
            for i, x in enumerate(v):
                o[0, i] = x
            v = o
        if isinstance(v, (bool, np.bool_)):
            v = np.array([[v]], dtype=np.bool_)
        elif isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, np.uint64):
            v = np.array([[v]], dtype=np.float64)
        v = np.asarray(v)
        if v.ndim == 0:
            v = v.reshape(1, 1)
        elif v.ndim == 1:
            v = v.reshape(1, -1)
        dims = (C.c_size_t * v.ndim)(*v.shape)
        if v.dtype == object:
            assert v.ndim == 2
            c = d.mxCreateCellMatrix(v.shape[0], v.shape[1])
            for i, x in enumerate(v.reshape(-1, order="F")):
                if x is not None:
                    d.mxSetCell(c, i, self.to_mx(x))
            return c
        if v.dtype not in _CLASS:
            raise TypeError("no mxArray class for dtype %s (convert to float64 first, as MATLAB would hold it)" % v.dtype)
        a = d.rt_new(_CLASS[v.dtype], v.ndim, dims)
        if v.size:
            flat = np.ascontiguousarray(v.reshape(-1, order="F"))
            C.memmove(d.mxGetData(a), flat.ctypes.data, flat.nbytes)
        return a

    # ---- mxArray -> numpy
    def from_mx(self, a):
        d = self.dll
        if not a:
            return None
        cls = d.rt_class(a)
        dims = tuple(int(d.rt_dim(a, i)) for i in range(d.rt_ndim(a)))
        n = int(np.prod(dims))
        if cls == CELL:
            out = np.empty(n, dtype=object)
            for i in range(n):
                out[i] = self.from_mx(d.mxGetCell(a, i))
            return out.reshape(dims, order="F")
        if cls == STRUCT:
            assert dims == (1, 1)
            return {d.rt_fieldname(a, f).decode(): self.from_mx(d.mxGetField(a, 0, d.rt_fieldname(a, f))) for f in range(d.rt_nfields(a))}
        dt = np.dtype(_DTYPE[cls])
        flat = np.empty(n, dtype=dt)
        if n:
            C.memmove(flat.ctypes.data, d.mxGetData(a), n * dt.itemsize)
        if cls == CHAR:
            assert dims[0] <= 1
            return "".join(chr(c) for c in flat)
        return flat.reshape(dims, order="F")

    def check(self, what=""):
        """The runtime's own record: overwritten guard words and API misuse (an index outside an array, a result slot beyond nlhs ...)."""
        bad = self.dll.rt_check_guards()
        n, text = self.dll.rt_violation_count(), (self.dll.rt_violations() or b"").decode()
        self.dll.rt_clear_violations()
        assert bad == 0 and n == 0, "%s: %d overwritten block(s), %d violation(s):\n%s" % (what, bad, n, text)

    def call(self, cmd, *args, nlhs=1):
        """emgpu_mex(cmd, args...) with nlhs outputs: the converted outputs (one value for nlhs <= 1, else a tuple), MexError on a gateway
        error.  Inputs and outputs are destroyed afterwards, and the runtime must hold no array and no block that this call made."""
        return self.call_raw([cmd] + list(args), nlhs=nlhs)

    def call_raw(self, args, nlhs=1):
        """call() with the command as args[0] (or with no argument at all)."""
        d = self.dll
        cmd = args[0] if args and isinstance(args[0], str) else "?"
        before = (d.rt_live_arrays(), d.rt_live_blocks())
        ins = [self.to_mx(a) for a in args]
        prhs = (C.c_void_p * max(len(ins), 1))(*ins)
        plhs = (C.c_void_p * MAX_OUT)()
        assert nlhs <= MAX_OUT
        rc = d.rt_call(nlhs, plhs, len(ins), prhs)
        try:
            self.check("emgpu_mex('%s', ...)" % cmd)
            if rc:
                raise MexError(d.rt_error_id().decode(), d.rt_error_msg().decode("latin-1"))
            outs = tuple(self.from_mx(plhs[k]) for k in range(max(nlhs, 1)))
        finally:
            for a in ins:
                d.rt_destroy(a)
            seen = set()
            for k in range(max(nlhs, 1)):
                if plhs[k] and plhs[k] not in seen:
                    seen.add(plhs[k])
                    d.rt_destroy(plhs[k])
        after = (d.rt_live_arrays(), d.rt_live_blocks())
        assert after == before, "emgpu_mex('%s', ...) left arrays / blocks behind: %r -> %r" % (cmd, before, after)
        self.check("after emgpu_mex('%s', ...)" % cmd)
        if nlhs == 0:
            return outs[0]        # MATLAB's `ans`: None for a command that returns nothing
        return outs[0] if nlhs == 1 else outs[:nlhs]

    def run_at_exit(self):
        """What clearing the mex file does: call the function the gateway registered with mexAtExit (it frees the gateway's contexts)."""
        return bool(self.dll.rt_run_at_exit())


def handle(h):
    """A model handle as the gateway returns it (1 x 1 uint64) -> the integer address, for ctypes calls on the same native model."""
    return int(np.asarray(h).reshape(-1)[0])
