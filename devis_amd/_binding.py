"""What the ctypes bindings of the mask-path operators share (``_mdcn``, ``_attmap``, ``_mhstage``, ``_maskloss``, ``_maskiou``, ``_maskrle``, ``_maskbiou``, ``_boxmatch``, ``_assign``, ``_labelloss``, ``_posembed``, ``_addnorm``, ``_selfattn``, ``_winattn``, ``_prenorm``, ``_frozennorm``, ``_swinends``, ``_inputproj``): how an
operator's entry points of libmsda_hip.so are checked and given their prototypes once, and how a failing call raises.
"""
import ctypes
import threading

from . import _native


def bind(prefix, abi_version, symbols, prototypes):
    """``(load, check)`` of the operator whose symbols start with ``prefix``.

    ``load()`` returns the library ``_native.load()`` opens, after checking once (under a lock) that it exports every
    name in ``symbols`` and that ``<prefix>_version()`` is ``abi_version``, and after ``prototypes(lib)`` has set restype /
    argtypes of the other entry points; it raises RuntimeError otherwise.  ``check(rc, what)`` returns ``rc``, or raises
    with ``<prefix>_last_error()`` when it is negative."""
    lock = threading.Lock()
    cached = []

    def load():
        if cached:
            return cached[0]
        with lock:
            if cached:
                return cached[0]
            lib = _native.load()
            for name in symbols:
                if not hasattr(lib, name):
                    raise RuntimeError("devis_amd: the HIP library does not export %s; rebuild with "
                                       "python -m devis_amd.build --force" % name)
            version, last_error = getattr(lib, prefix + "_version"), getattr(lib, prefix + "_last_error")
            version.restype = ctypes.c_int
            last_error.restype = ctypes.c_char_p
            if version() != abi_version:
                raise RuntimeError("devis_amd: %s ABI version mismatch (library %d, binding %d); rebuild with "
                                   "python -m devis_amd.build --force" % (prefix, version(), abi_version))
            prototypes(lib)
            cached.append(lib)
        return cached[0]

    def check(rc, what):
        if rc < 0:
            msg = getattr(load(), prefix + "_last_error")().decode("utf-8", "replace")
            raise RuntimeError("devis_amd: %s failed (status %d): %s" % (what, rc, msg))
        return rc

    return load, check
