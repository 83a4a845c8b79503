"""Locate, build and load libwsframe_amd.so (in-tree, next to this file).

Fails loudly: there is no Python or CPU fallback for the batch path.
"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
# (WSFRAME_AMD_LIB: another build of the same library, for A/B measurements only)
LIB_PATH = os.environ.get("WSFRAME_AMD_LIB") or os.path.join(HERE, "libwsframe_amd.so")
# bench / test support (synthetic batches generated in HBM, calibration): NOT the drop-in
BENCH_LIB_PATH = os.path.join(HERE, "libwsframe_amd_bench.so")
_lib = None
_bench = None


class WsDesc(C.Structure):
    _fields_ = [("frame_off", C.c_ulonglong), ("data_off", C.c_ulonglong), ("datalen", C.c_ulonglong),
                ("ret", C.c_int), ("is_fin", C.c_ubyte), ("type", C.c_ubyte), ("masked", C.c_ubyte),
                ("hdrlen", C.c_ubyte)]


class WsSegRes(C.Structure):
    _fields_ = [("consumed", C.c_ulonglong), ("n_frames", C.c_uint), ("status", C.c_int)]


# the reference's eight symbols (inc/crt/protocol/websocketframe.h:42-49)
REFERENCE_EXPORTS = [
    "websocketframeComputeSecAccept", "websocketframeDecodeHandshakeRequest",
    "websocketframeEncodeHandshakeResponse", "websocketframeEncodeHandshakeResponseWithProtocol",
    "websocketframeFreeString", "websocketframeDecode", "websocketframeEncodeHeadLength",
    "websocketframeEncode",
]
# every symbol include/wsframe_amd.h + include/wsframe_amd_channel.h declare: the whole
# dynamic symbol table of libwsframe_amd.so
EXPORTS = REFERENCE_EXPORTS + [
    "websocketframeBatchDecodeDevice", "websocketframeBatchDecodeHost", "websocketframeBatchDecodeHostMulti",
    "websocketframeBatchEncodeDevice", "websocketframeBatchReassembleDevice",
    "websocketframeBatchReassembleDeviceEx", "websocketframeStreamDecodeDevice",
    "websocketframeGpuLastError", "websocketframeGpuSetOption", "websocketframeGpuGetStat",
    "websocketframeOnDecode", "websocketframeOnDecodeBatch",
]
# libwsframe_amd_ctl.so: the same objects, with the WSFRAME_AMD_CTL_EXPORT entry points exported too
CTL_LIB_PATH = os.path.join(HERE, "libwsframe_amd_ctl.so")
CTL_EXPORTS = ["websocketframeBatchReassembleDeviceCtl", "websocketframeOnDecodeControl",
               "websocketframeOnDecodeBatchControl"]
_ctl = None
# libwsframe_amd_text.so: everything libwsframe_amd_ctl.so exports plus the WSFRAME_AMD_TEXT_EXPORT
# entry point (include/wsframe_amd_text.h)
TEXT_LIB_PATH = os.path.join(HERE, "libwsframe_amd_text.so")
TEXT_EXPORTS = ["websocketframeBatchValidateTextDevice"]
_text = None
# libwsframe_amd_proto.so: everything libwsframe_amd_text.so exports plus the WSFRAME_AMD_PROTO_EXPORT
# entry points (include/wsframe_amd_proto.h)
PROTO_LIB_PATH = os.path.join(HERE, "libwsframe_amd_proto.so")
PROTO_EXPORTS = ["websocketframeBatchCheckProtocolDevice", "websocketframeProtoStepHost"]
_proto = None
# libwsframe_amd_hs.so: everything libwsframe_amd_proto.so exports plus the WSFRAME_AMD_HS_EXPORT
# entry points (include/wsframe_amd_handshake.h)
HS_LIB_PATH = os.path.join(HERE, "libwsframe_amd_hs.so")
HS_EXPORTS = ["websocketframeBatchHandshakeDevice", "websocketframeHandshakeHost"]
_hs = None
# libwsframe_amd_reply.so: everything libwsframe_amd_hs.so exports plus the WSFRAME_AMD_REPLY_EXPORT
# entry points (include/wsframe_amd_reply.h)
REPLY_LIB_PATH = os.path.join(HERE, "libwsframe_amd_reply.so")
REPLY_EXPORTS = ["websocketframeBatchControlRepliesDevice", "websocketframeControlRepliesHost"]
_reply = None
# libwsframe_amd_send.so: everything libwsframe_amd_reply.so exports plus the WSFRAME_AMD_SEND_EXPORT
# entry points (include/wsframe_amd_send.h)
SEND_LIB_PATH = os.path.join(HERE, "libwsframe_amd_send.so")
SEND_EXPORTS = ["websocketframeBatchSendDevice", "websocketframeBatchSendListFromMessagesDevice",
                "websocketframeSendHost"]
_send = None
# libwsframe_amd_cli.so: everything libwsframe_amd_send.so exports plus the WSFRAME_AMD_CLI_EXPORT
# entry points (include/wsframe_amd_client.h)
CLI_LIB_PATH = os.path.join(HERE, "libwsframe_amd_cli.so")
CLI_EXPORTS = ["websocketframeBatchClientRequestDevice", "websocketframeBatchClientVerifyDevice",
               "websocketframeClientRequestHost", "websocketframeClientVerifyHost"]
_cli = None
# libwsframe_amd_deflate.so: everything libwsframe_amd_cli.so exports plus the WSFRAME_AMD_DEFLATE_EXPORT
# entry points (include/wsframe_amd_deflate.h)
DEFLATE_LIB_PATH = os.path.join(HERE, "libwsframe_amd_deflate.so")
DEFLATE_EXPORTS = ["websocketframeBatchInflateDevice", "websocketframeBatchInflateListFromMessagesDevice",
                   "websocketframeInflateHost"]
_deflate = None
# libwsframe_amd_pmd.so: everything libwsframe_amd_deflate.so exports plus the WSFRAME_AMD_PMD_EXPORT
# entry points (include/wsframe_amd_compress.h)
PMD_LIB_PATH = os.path.join(HERE, "libwsframe_amd_pmd.so")
PMD_EXPORTS = ["websocketframeBatchDeflateDevice", "websocketframeBatchSendListFromDeflatedDevice",
               "websocketframeBatchSendExtDevice", "websocketframeDeflateHost", "websocketframeSendExtHost"]
_pmd = None
_options = {}            # options set through set_option(): the ctl, text, proto, hs, reply, send, cli, deflate and pmd libraries keep their own copies
# include/wsframe_amd_bench.h (libwsframe_amd_bench.so)
BENCH_EXPORTS = ["websocketframeSynthDevice", "websocketframeSynthVerifyDevice", "websocketframeGpuCalibrate",
                 "websocketframeBenchLastError", "websocketframeSynthDeviceRange",
                 "websocketframeSynthVerifyDeviceRange", "websocketframeFrameHashDevice",
                 "websocketframeBenchAlloc", "websocketframeBenchFree", "websocketframeBenchTorchAlloc",
                 "websocketframeBenchTorchFree"]


def build_lib(force=False):
    """make -C util_amd/csrc (hipcc --offload-arch=gfx950 + gcc)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(HERE, "csrc")] + (["-B"] if force else []), check=True)
    return LIB_PATH


def _one_hip_runtime():
    """Load torch (when installed) before our libraries: torch's ROCm wheel carries its own
    libamdhip64 (soname libamdhip64.so.7, NEEDED as "libamdhip64.so"), so a library of ours
    loaded first would pull /opt/rocm's copy in and the process would hold two HIP runtimes
    (kernels of the second one then see no device). Loaded after torch, ours bind to torch's."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def load_lib():
    global _lib
    if _lib is not None:
        return _lib
    _one_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libwsframe_amd.so not built: run __graft_entry__.build() "
                           "(make -C util_amd/csrc); there is no fallback path")
    lib = C.CDLL(LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_ulonglong, C.c_uint, C.c_int
    P = C.POINTER
    lib.websocketframeDecode.restype = i32
    lib.websocketframeDecode.argtypes = [vp, u64, P(vp), P(u64), P(i32), P(i32)]
    lib.websocketframeEncodeHeadLength.restype = u32
    lib.websocketframeEncodeHeadLength.argtypes = [u64]
    lib.websocketframeEncode.restype = None
    lib.websocketframeEncode.argtypes = [vp, i32, i32, i32, u64]
    lib.websocketframeComputeSecAccept.restype = vp
    lib.websocketframeComputeSecAccept.argtypes = [C.c_char_p, u32, vp]
    lib.websocketframeDecodeHandshakeRequest.restype = i32
    lib.websocketframeDecodeHandshakeRequest.argtypes = [vp, u32, P(vp), P(u32), P(vp), P(u32)]
    lib.websocketframeEncodeHandshakeResponse.restype = vp
    lib.websocketframeEncodeHandshakeResponse.argtypes = [C.c_char_p, u32, vp]
    lib.websocketframeEncodeHandshakeResponseWithProtocol.restype = vp
    lib.websocketframeEncodeHandshakeResponseWithProtocol.argtypes = [C.c_char_p, u32, C.c_char_p, u32]
    lib.websocketframeFreeString.restype = None
    lib.websocketframeFreeString.argtypes = [vp]
    lib.websocketframeBatchDecodeDevice.restype = i32
    lib.websocketframeBatchDecodeDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp]
    lib.websocketframeBatchReassembleDevice.restype = i32
    lib.websocketframeBatchReassembleDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.websocketframeStreamDecodeDevice.restype = i32
    lib.websocketframeStreamDecodeDevice.argtypes = [vp, u64, u32, vp, vp, vp]
    lib.websocketframeBatchEncodeDevice.restype = i32
    lib.websocketframeBatchEncodeDevice.argtypes = [vp, vp, u32, vp, u64, vp, vp]
    lib.websocketframeBatchDecodeHost.restype = i32
    lib.websocketframeBatchDecodeHost.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, i32]
    lib.websocketframeBatchDecodeHostMulti.restype = i32
    lib.websocketframeBatchDecodeHostMulti.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, i32]
    lib.websocketframeGpuLastError.restype = C.c_char_p
    lib.websocketframeGpuLastError.argtypes = []
    lib.websocketframeGpuSetOption.restype = i32
    lib.websocketframeGpuSetOption.argtypes = [C.c_char_p, C.c_longlong]
    lib.websocketframeGpuGetStat.restype = i32
    lib.websocketframeGpuGetStat.argtypes = [C.c_char_p, P(C.c_ulonglong)]
    lib.websocketframeBatchReassembleDeviceEx.restype = i32
    lib.websocketframeBatchReassembleDeviceEx.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp,
                                                          vp]
    lib.websocketframeOnDecode.restype = None
    lib.websocketframeOnDecode.argtypes = [vp, vp, C.c_size_t, vp]
    lib.websocketframeOnDecodeBatch.restype = None
    lib.websocketframeOnDecodeBatch.argtypes = [vp, vp, C.c_size_t, vp]
    _env_options(lib)
    _lib = lib
    return lib


def _env_options(lib):
    """launch tuning from the environment, e.g. WSFRAME_AMD_OPTIONS=path=0,seg_cfg=10"""
    for kv in filter(None, os.environ.get("WSFRAME_AMD_OPTIONS", "").split(",")):
        name, _, value = kv.partition("=")
        if lib.websocketframeGpuSetOption(name.strip().encode(), int(value)) != 0:
            raise ValueError("WSFRAME_AMD_OPTIONS: unknown option %r" % name)


def set_option(name, value):
    """websocketframeGpuSetOption on libwsframe_amd.so and, once loaded, on libwsframe_amd_ctl.so
    (options are per library: the two do not share state). Returns the C return code."""
    rc = load_lib().websocketframeGpuSetOption(name.encode(), int(value))
    if rc == 0:
        _options[name] = int(value)
        if _ctl is not None:
            _ctl.websocketframeGpuSetOption(name.encode(), int(value))
        if _text is not None:
            _text.websocketframeGpuSetOption(name.encode(), int(value))
        if _proto is not None:
            _proto.websocketframeGpuSetOption(name.encode(), int(value))
        if _hs is not None:
            _hs.websocketframeGpuSetOption(name.encode(), int(value))
        if _reply is not None:
            _reply.websocketframeGpuSetOption(name.encode(), int(value))
        if _send is not None:
            _send.websocketframeGpuSetOption(name.encode(), int(value))
        if _cli is not None:
            _cli.websocketframeGpuSetOption(name.encode(), int(value))
        if _deflate is not None:
            _deflate.websocketframeGpuSetOption(name.encode(), int(value))
        if _pmd is not None:
            _pmd.websocketframeGpuSetOption(name.encode(), int(value))
    return rc


def load_ctl_lib():
    """libwsframe_amd_ctl.so: websocketframeBatchReassembleDeviceCtl and the control-direct glue.
    A library of its own state (workspace, options, last error): the options set so far through
    set_option() are applied when it loads and forwarded afterwards."""
    global _ctl
    if _ctl is not None:
        return _ctl
    load_lib()
    if not os.path.exists(CTL_LIB_PATH):
        raise RuntimeError("libwsframe_amd_ctl.so not built: run __graft_entry__.build(); there is no fallback path")
    lib = C.CDLL(CTL_LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_ulonglong, C.c_uint, C.c_int
    lib.websocketframeBatchReassembleDeviceCtl.restype = i32
    lib.websocketframeBatchReassembleDeviceCtl.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp,
                                                           u32, vp]
    lib.websocketframeOnDecodeControl.restype = None
    lib.websocketframeOnDecodeControl.argtypes = [vp, vp, C.c_size_t, vp]
    lib.websocketframeOnDecodeBatchControl.restype = None
    lib.websocketframeOnDecodeBatchControl.argtypes = [vp, vp, C.c_size_t, vp]
    lib.websocketframeGpuLastError.restype = C.c_char_p
    lib.websocketframeGpuLastError.argtypes = []
    lib.websocketframeGpuSetOption.restype = i32
    lib.websocketframeGpuSetOption.argtypes = [C.c_char_p, C.c_longlong]
    _env_options(lib)
    for name, value in _options.items():
        lib.websocketframeGpuSetOption(name.encode(), value)
    _ctl = lib
    return lib


def load_text_lib():
    """libwsframe_amd_text.so: websocketframeBatchValidateTextDevice next to the whole C ABI of
    libwsframe_amd_ctl.so (one library for a text server). A library of its own state, as
    load_ctl_lib(): the options set so far are applied when it loads and forwarded afterwards."""
    global _text
    if _text is not None:
        return _text
    load_lib()
    if not os.path.exists(TEXT_LIB_PATH):
        raise RuntimeError("libwsframe_amd_text.so not built: run __graft_entry__.build(); there is no fallback path")
    lib = C.CDLL(TEXT_LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_ulonglong, C.c_uint, C.c_int
    lib.websocketframeBatchValidateTextDevice.restype = i32
    lib.websocketframeBatchValidateTextDevice.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, vp, vp]
    lib.websocketframeBatchReassembleDevice.restype = i32
    lib.websocketframeBatchReassembleDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.websocketframeBatchReassembleDeviceEx.restype = i32
    lib.websocketframeBatchReassembleDeviceEx.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp,
                                                          vp]
    lib.websocketframeBatchReassembleDeviceCtl.restype = i32
    lib.websocketframeBatchReassembleDeviceCtl.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp,
                                                           u32, vp]
    lib.websocketframeGpuLastError.restype = C.c_char_p
    lib.websocketframeGpuLastError.argtypes = []
    lib.websocketframeGpuSetOption.restype = i32
    lib.websocketframeGpuSetOption.argtypes = [C.c_char_p, C.c_longlong]
    lib.websocketframeGpuGetStat.restype = i32
    lib.websocketframeGpuGetStat.argtypes = [C.c_char_p, C.POINTER(C.c_ulonglong)]
    _env_options(lib)
    for name, value in _options.items():
        lib.websocketframeGpuSetOption(name.encode(), value)
    _text = lib
    return lib


def load_proto_lib():
    """libwsframe_amd_proto.so: websocketframeBatchCheckProtocolDevice and websocketframeProtoStepHost
    next to the whole C ABI of libwsframe_amd_text.so (decode, reassembly, text validation and the
    protocol check on one workspace). A library of its own state, as load_text_lib(): the options
    set so far are applied when it loads and forwarded afterwards."""
    global _proto
    if _proto is not None:
        return _proto
    load_lib()
    if not os.path.exists(PROTO_LIB_PATH):
        raise RuntimeError("libwsframe_amd_proto.so not built: run __graft_entry__.build(); there is no fallback path")
    lib = C.CDLL(PROTO_LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_ulonglong, C.c_uint, C.c_int
    lib.websocketframeBatchCheckProtocolDevice.restype = i32
    lib.websocketframeBatchCheckProtocolDevice.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, u64, vp, vp, vp, vp]
    lib.websocketframeProtoStepHost.restype = i32
    lib.websocketframeProtoStepHost.argtypes = [C.POINTER(u64), C.c_ubyte, i32, u64, C.c_char_p, u32, u32, u64]
    lib.websocketframeBatchDecodeDevice.restype = i32
    lib.websocketframeBatchDecodeDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp]
    lib.websocketframeStreamDecodeDevice.restype = i32
    lib.websocketframeStreamDecodeDevice.argtypes = [vp, u64, u32, vp, vp, vp]
    lib.websocketframeBatchReassembleDeviceCtl.restype = i32
    lib.websocketframeBatchReassembleDeviceCtl.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp,
                                                           u32, vp]
    lib.websocketframeGpuLastError.restype = C.c_char_p
    lib.websocketframeGpuLastError.argtypes = []
    lib.websocketframeGpuSetOption.restype = i32
    lib.websocketframeGpuSetOption.argtypes = [C.c_char_p, C.c_longlong]
    lib.websocketframeGpuGetStat.restype = i32
    lib.websocketframeGpuGetStat.argtypes = [C.c_char_p, C.POINTER(C.c_ulonglong)]
    _env_options(lib)
    for name, value in _options.items():
        lib.websocketframeGpuSetOption(name.encode(), value)
    _proto = lib
    return lib


def load_hs_lib():
    """libwsframe_amd_hs.so: websocketframeBatchHandshakeDevice and websocketframeHandshakeHost next to
    the whole C ABI of libwsframe_amd_proto.so (a connection from its upgrade request to its close
    on one library). A library of its own state, as load_proto_lib(): the options set so far are
    applied when it loads and forwarded afterwards."""
    global _hs
    if _hs is not None:
        return _hs
    load_lib()
    if not os.path.exists(HS_LIB_PATH):
        raise RuntimeError("libwsframe_amd_hs.so not built: run __graft_entry__.build(); there is no fallback path")
    lib = C.CDLL(HS_LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_ulonglong, C.c_uint, C.c_int
    lib.websocketframeBatchHandshakeDevice.restype = i32
    lib.websocketframeBatchHandshakeDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, u32, vp]
    lib.websocketframeHandshakeHost.restype = i32
    lib.websocketframeHandshakeHost.argtypes = [vp, u32, u32, vp, vp, vp, u32]
    lib.websocketframeBatchDecodeDevice.restype = i32
    lib.websocketframeBatchDecodeDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp]
    lib.websocketframeGpuLastError.restype = C.c_char_p
    lib.websocketframeGpuLastError.argtypes = []
    lib.websocketframeGpuSetOption.restype = i32
    lib.websocketframeGpuSetOption.argtypes = [C.c_char_p, C.c_longlong]
    _env_options(lib)
    for name, value in _options.items():
        lib.websocketframeGpuSetOption(name.encode(), value)
    _hs = lib
    return lib


def load_reply_lib():
    """libwsframe_amd_reply.so: websocketframeBatchControlRepliesDevice and
    websocketframeControlRepliesHost next to the whole C ABI of libwsframe_amd_hs.so (decode, check,
    reply on one workspace). A library of its own state, as load_hs_lib(): the options set so far
    are applied when it loads and forwarded afterwards."""
    global _reply
    if _reply is not None:
        return _reply
    load_lib()
    if not os.path.exists(REPLY_LIB_PATH):
        raise RuntimeError("libwsframe_amd_reply.so not built: run __graft_entry__.build(); there is no fallback path")
    lib = C.CDLL(REPLY_LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_ulonglong, C.c_uint, C.c_int
    lib.websocketframeBatchControlRepliesDevice.restype = i32
    lib.websocketframeBatchControlRepliesDevice.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, u64, vp, vp, vp]
    lib.websocketframeControlRepliesHost.restype = C.c_longlong
    lib.websocketframeControlRepliesHost.argtypes = [vp, u64, vp, vp, u32, u32, vp, u32, vp, vp, vp, u64, vp]
    lib.websocketframeBatchCheckProtocolDevice.restype = i32
    lib.websocketframeBatchCheckProtocolDevice.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, u64, vp, vp, vp, vp]
    lib.websocketframeBatchDecodeDevice.restype = i32
    lib.websocketframeBatchDecodeDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp]
    lib.websocketframeStreamDecodeDevice.restype = i32
    lib.websocketframeStreamDecodeDevice.argtypes = [vp, u64, u32, vp, vp, vp]
    lib.websocketframeBatchReassembleDeviceCtl.restype = i32
    lib.websocketframeBatchReassembleDeviceCtl.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp,
                                                           u32, vp]
    lib.websocketframeGpuLastError.restype = C.c_char_p
    lib.websocketframeGpuLastError.argtypes = []
    lib.websocketframeGpuSetOption.restype = i32
    lib.websocketframeGpuSetOption.argtypes = [C.c_char_p, C.c_longlong]
    lib.websocketframeGpuGetStat.restype = i32
    lib.websocketframeGpuGetStat.argtypes = [C.c_char_p, C.POINTER(C.c_ulonglong)]
    _env_options(lib)
    for name, value in _options.items():
        lib.websocketframeGpuSetOption(name.encode(), value)
    _reply = lib
    return lib


def load_send_lib():
    """libwsframe_amd_send.so: websocketframeBatchSendDevice, websocketframeBatchSendListFromMessagesDevice
    and websocketframeSendHost next to the whole C ABI of libwsframe_amd_reply.so (receive, reply and
    send on one workspace). A library of its own state, as load_reply_lib(): the options set so far
    are applied when it loads and forwarded afterwards."""
    global _send
    if _send is not None:
        return _send
    load_lib()
    if not os.path.exists(SEND_LIB_PATH):
        raise RuntimeError("libwsframe_amd_send.so not built: run __graft_entry__.build(); there is no fallback path")
    lib = C.CDLL(SEND_LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_ulonglong, C.c_uint, C.c_int
    lib.websocketframeBatchSendDevice.restype = i32
    lib.websocketframeBatchSendDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, u32, vp, u64, vp, vp, vp, vp]
    lib.websocketframeBatchSendListFromMessagesDevice.restype = i32
    lib.websocketframeBatchSendListFromMessagesDevice.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    lib.websocketframeSendHost.restype = C.c_longlong
    lib.websocketframeSendHost.argtypes = [vp, u64, vp, u32, u32, vp, u32, vp, u64, vp, vp]
    lib.websocketframeGpuLastError.restype = C.c_char_p
    lib.websocketframeGpuLastError.argtypes = []
    lib.websocketframeGpuSetOption.restype = i32
    lib.websocketframeGpuSetOption.argtypes = [C.c_char_p, C.c_longlong]
    _env_options(lib)
    for name, value in _options.items():
        lib.websocketframeGpuSetOption(name.encode(), value)
    _send = lib
    return lib


def load_cli_lib():
    """libwsframe_amd_cli.so: the client handshake (websocketframeBatchClientRequestDevice,
    websocketframeBatchClientVerifyDevice and their host twins) next to the whole C ABI of
    libwsframe_amd_send.so (a connection opened in either role on one library). A library of its
    own state, as load_send_lib(): the options set so far are applied when it loads and forwarded
    afterwards."""
    global _cli
    if _cli is not None:
        return _cli
    load_lib()
    if not os.path.exists(CLI_LIB_PATH):
        raise RuntimeError("libwsframe_amd_cli.so not built: run __graft_entry__.build(); there is no fallback path")
    lib = C.CDLL(CLI_LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_ulonglong, C.c_uint, C.c_int
    lib.websocketframeBatchClientRequestDevice.restype = i32
    lib.websocketframeBatchClientRequestDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, u32, vp, vp, vp]
    lib.websocketframeBatchClientVerifyDevice.restype = i32
    lib.websocketframeBatchClientVerifyDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, u64, vp, u32, vp, vp]
    lib.websocketframeClientRequestHost.restype = i32
    lib.websocketframeClientRequestHost.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp, vp]
    lib.websocketframeClientVerifyHost.restype = i32
    lib.websocketframeClientVerifyHost.argtypes = [vp, u32, u32, vp, vp, u32, u32, vp]
    lib.websocketframeBatchHandshakeDevice.restype = i32
    lib.websocketframeBatchHandshakeDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, u32, vp]
    lib.websocketframeBatchDecodeDevice.restype = i32
    lib.websocketframeBatchDecodeDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp]
    lib.websocketframeGpuLastError.restype = C.c_char_p
    lib.websocketframeGpuLastError.argtypes = []
    lib.websocketframeGpuSetOption.restype = i32
    lib.websocketframeGpuSetOption.argtypes = [C.c_char_p, C.c_longlong]
    _env_options(lib)
    for name, value in _options.items():
        lib.websocketframeGpuSetOption(name.encode(), value)
    _cli = lib
    return lib


def load_deflate_lib():
    """libwsframe_amd_deflate.so: the permessage-deflate receive side (websocketframeBatchInflateDevice,
    websocketframeBatchInflateListFromMessagesDevice, websocketframeInflateHost) next to the whole C
    ABI of libwsframe_amd_cli.so. A library of its own state, as load_cli_lib(): the options set so
    far are applied when it loads and forwarded afterwards."""
    global _deflate
    if _deflate is not None:
        return _deflate
    load_lib()
    if not os.path.exists(DEFLATE_LIB_PATH):
        raise RuntimeError("libwsframe_amd_deflate.so not built: run __graft_entry__.build(); there is no fallback path")
    lib = C.CDLL(DEFLATE_LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_ulonglong, C.c_uint, C.c_int
    lib.websocketframeBatchInflateDevice.restype = i32
    lib.websocketframeBatchInflateDevice.argtypes = [vp, u64, vp, vp, u32, u32, u64, u32, vp, vp, vp, vp, vp, vp]
    lib.websocketframeBatchInflateListFromMessagesDevice.restype = i32
    lib.websocketframeBatchInflateListFromMessagesDevice.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp]
    lib.websocketframeInflateHost.restype = C.c_longlong
    lib.websocketframeInflateHost.argtypes = [vp, u64, vp, u32, u64, u32, vp, u64, vp, vp]
    lib.websocketframeGpuLastError.restype = C.c_char_p
    lib.websocketframeGpuLastError.argtypes = []
    lib.websocketframeGpuSetOption.restype = i32
    lib.websocketframeGpuSetOption.argtypes = [C.c_char_p, C.c_longlong]
    _env_options(lib)
    for name, value in _options.items():
        lib.websocketframeGpuSetOption(name.encode(), value)
    _deflate = lib
    return lib


def load_pmd_lib():
    """libwsframe_amd_pmd.so: the permessage-deflate send side (websocketframeBatchDeflateDevice,
    websocketframeBatchSendListFromDeflatedDevice, websocketframeBatchSendExtDevice and the host twins
    websocketframeDeflateHost, websocketframeSendExtHost) next to the whole C ABI of
    libwsframe_amd_deflate.so. A library of its own state, as load_deflate_lib(): the options set so
    far are applied when it loads and forwarded afterwards."""
    global _pmd
    if _pmd is not None:
        return _pmd
    load_lib()
    if not os.path.exists(PMD_LIB_PATH):
        raise RuntimeError("libwsframe_amd_pmd.so not built: run __graft_entry__.build(); there is no fallback path")
    lib = C.CDLL(PMD_LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_ulonglong, C.c_uint, C.c_int
    lib.websocketframeBatchDeflateDevice.restype = i32
    lib.websocketframeBatchDeflateDevice.argtypes = [vp, u64, vp, vp, u32, u32, u64, u32, vp, vp, vp, vp, vp]
    lib.websocketframeBatchSendListFromDeflatedDevice.restype = i32
    lib.websocketframeBatchSendListFromDeflatedDevice.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    lib.websocketframeBatchSendExtDevice.restype = i32
    lib.websocketframeBatchSendExtDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, u32, vp, u64, vp, vp, vp, vp]
    lib.websocketframeDeflateHost.restype = C.c_longlong
    lib.websocketframeDeflateHost.argtypes = [vp, u64, vp, u32, u64, u32, vp, vp, vp, vp]
    lib.websocketframeSendExtHost.restype = C.c_longlong
    lib.websocketframeSendExtHost.argtypes = [vp, u64, vp, u32, u32, vp, u32, vp, u64, vp, vp]
    lib.websocketframeBatchSendDevice.restype = i32
    lib.websocketframeBatchSendDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, u32, vp, u64, vp, vp, vp, vp]
    lib.websocketframeSendHost.restype = C.c_longlong
    lib.websocketframeSendHost.argtypes = [vp, u64, vp, u32, u32, vp, u32, vp, u64, vp, vp]
    lib.websocketframeBatchReassembleDevice.restype = i32
    lib.websocketframeBatchReassembleDevice.argtypes = [vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.websocketframeBatchInflateDevice.restype = i32
    lib.websocketframeBatchInflateDevice.argtypes = [vp, u64, vp, vp, u32, u32, u64, u32, vp, vp, vp, vp, vp, vp]
    lib.websocketframeBatchInflateListFromMessagesDevice.restype = i32
    lib.websocketframeBatchInflateListFromMessagesDevice.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp]
    lib.websocketframeInflateHost.restype = C.c_longlong
    lib.websocketframeInflateHost.argtypes = [vp, u64, vp, u32, u64, u32, vp, u64, vp, vp]
    lib.websocketframeGpuLastError.restype = C.c_char_p
    lib.websocketframeGpuLastError.argtypes = []
    lib.websocketframeGpuSetOption.restype = i32
    lib.websocketframeGpuSetOption.argtypes = [C.c_char_p, C.c_longlong]
    _env_options(lib)
    for name, value in _options.items():
        lib.websocketframeGpuSetOption(name.encode(), value)
    _pmd = lib
    return lib


def load_bench_lib():
    """libwsframe_amd_bench.so: synthetic batches in HBM + calibration kernels (bench/tests)"""
    global _bench
    if _bench is not None:
        return _bench
    _one_hip_runtime()
    if not os.path.exists(BENCH_LIB_PATH):
        raise RuntimeError("libwsframe_amd_bench.so not built: run __graft_entry__.build()")
    lib = C.CDLL(BENCH_LIB_PATH)
    vp, u64, i32 = C.c_void_p, C.c_ulonglong, C.c_int
    lib.websocketframeGpuCalibrate.restype = i32
    lib.websocketframeGpuCalibrate.argtypes = [vp, vp, u64, i32, i32, i32, vp]
    lib.websocketframeSynthDevice.restype = i32
    lib.websocketframeSynthDevice.argtypes = [vp, vp, u64, i32, u64, i32, u64, vp]
    lib.websocketframeSynthVerifyDevice.restype = i32
    lib.websocketframeSynthVerifyDevice.argtypes = [vp, vp, u64, i32, u64, u64, i32, vp, vp]
    lib.websocketframeSynthDeviceRange.restype = i32
    lib.websocketframeSynthDeviceRange.argtypes = [vp, vp, u64, u64, i32, u64, i32, u64, vp]
    lib.websocketframeSynthVerifyDeviceRange.restype = i32
    lib.websocketframeSynthVerifyDeviceRange.argtypes = [vp, vp, u64, u64, i32, u64, u64, i32, vp, vp]
    lib.websocketframeFrameHashDevice.restype = i32
    lib.websocketframeFrameHashDevice.argtypes = [vp, vp, vp, C.c_uint, C.c_uint, vp, vp]
    lib.websocketframeBenchLastError.restype = C.c_char_p
    lib.websocketframeBenchLastError.argtypes = []
    _bench = lib
    return lib


def check(rc, what, lib=None):
    if rc != 0:
        err = (lib or load_lib()).websocketframeGpuLastError().decode(errors="replace")
        raise RuntimeError("%s failed (%d): %s" % (what, rc, err))


def check_bench(rc, what):
    if rc != 0:
        err = load_bench_lib().websocketframeBenchLastError().decode(errors="replace")
        raise RuntimeError("%s failed (%d): %s" % (what, rc, err))
