"""What the ctypes faces of the three libraries share (_lib, rbergomi, agent): the loader, and the
pointer and stream arguments of a device call.  Imports without torch and without a GPU."""
import ctypes
import os


def load(path, sig, error, no_fallback, missing_ok=False):
    """CDLL(path) with the restype / argtypes of `sig` = {symbol: (restype, argtypes)} applied.
    `error` is raised when the file is missing; missing_ok skips symbols an older build lacks.  torch
    is imported first so that the HIP runtime torch ships (SONAME libamdhip64.so.7) is the one the
    library binds to -- one runtime per process, so torch streams and data_ptr()s are valid here."""
    if not os.path.exists(path):
        raise error(f"{path} not found: build it with `python -m cantorrl_amd.build` "
                    f"(hipcc --offload-arch=gfx950).  {no_fallback}")
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    for name, (res, args) in sig.items():
        if missing_ok and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def ptr(t):
    """A tensor's device address as a pointer argument (a c_void_p); None stays None (NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream(device_index):
    """The raw handle of the caller's current stream on that device: torch's own accessor
    (current_stream().cuda_stream builds a Stream object per call, a few us of every eager step).
    The first call puts that accessor in this function's place, so `_bind.stream(i)` is then a
    direct call of it."""
    global stream
    import torch
    stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or \
        (lambda idx: torch.cuda.current_stream(idx).cuda_stream)
    return stream(device_index)


def stream_of(device):
    """stream() for a torch.device or its name ("cuda": the current device)."""
    import torch
    d = torch.device(device)
    return stream(d.index if d.index is not None else torch.cuda.current_device())
