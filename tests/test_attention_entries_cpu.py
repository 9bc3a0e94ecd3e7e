"""The six kernel-level attention entries and the two cache entries of include/m2fnet_hip.h on the host alone: every refusal comes before
any HIP call, so the entries are called here with dummy pointers (never dereferenced) and each refused argument must return non-zero with a
message that names the entry; and the two ctypes Structures of runtime.py must have the size and field offsets the library was compiled
with (m2f_attention_opts_layout)."""
import ctypes

import pytest

from mer_amd import runtime

P16, P4, P1 = 0x10000, 0x10004, 0x10001          # dummy device pointers: 16-byte aligned, 4-byte aligned only, unaligned
B, L, H, HD, E = 2, 8, 4, 8, 32
S, C, T, R = 2, 8, 2, 16


def _opts(**kw):
    return runtime.AttnOptsC(**dict(dict(past=-1, future=-1, bias_gain=0.0, n_same=0, n_other=0, speakers=None), **kw))


def _sopts(**kw):
    return runtime.AttnStreamOptsC(**kw)


def _paged(**kw):
    return _sopts(**dict(dict(table=P4, table_cols=1, n_pages=2, page_rows=R), **kw))


def _fwd(opts, **kw):
    a = dict(dict(B=B, L=L, H=H, hd=HD), **kw)
    return ("m2f_attention_fwd", (a["B"], a["L"], a["H"], a["hd"], P16, E, P16, E, P16, E, P16, P16, E, P16, 0, 0.0, None, None,
                                  ctypes.byref(opts) if opts is not None else None))


def _varlen(opts, bwd=False, **kw):
    a = dict(dict(B=B, L=L, H=H, hd=HD, cu=None, T=B * L, key_pad=P16), **kw)
    head = (a["B"], a["L"], a["H"], a["hd"], P16, E, P16, E, P16, E, a["cu"], a["T"], a["key_pad"], P16, E, P16)
    if bwd:
        return ("m2f_attention_varlen_bwd", head + (P16, E, P16, E, P16, E, P16, E, 0, 0.0, None, None, -1, -1))
    return ("m2f_attention_varlen_fwd", head + (0, 0.0, None, None, ctypes.byref(opts) if opts is not None else None))


def _stream(opts, chunk=False, **kw):
    a = dict(dict(S=S, T=T, H=H, hd=HD, q=P16, ld=E, kc=P16, vc=P16, C=C, count=P16, second=P16, out=P16), **kw)
    shape = (a["S"], a["T"], a["H"], a["hd"]) if chunk else (a["S"], a["H"], a["hd"])
    return ("m2f_attention_stream_chunk" if chunk else "m2f_attention_stream",
            shape + (a["q"], a["ld"], P16, E, P16, E, a["kc"], a["vc"], a["C"], 0, a["count"], a["second"], a["out"], E, 0, None,
                     ctypes.byref(opts) if opts is not None else None))


def _cache(scatter, **kw):
    a = dict(dict(S=S, H=H, hd=HD, kc=P16, vc=P16, table=None, table_cols=0, n_pages=0, page_rows=0, C=C, n=1, slots=P16, lengths=P16,
                  offsets=P16, packed=P16, elems=64, count=P16), **kw)
    args = (a["S"], a["H"], a["hd"], a["kc"], a["vc"], a["table"], a["table_cols"], a["n_pages"], a["page_rows"], a["C"], 0, a["n"], a["slots"],
            a["lengths"], a["offsets"], a["packed"], a["elems"])
    if scatter:
        return ("m2f_attention_stream_cache_scatter", args + (a["count"], None))
    return ("m2f_attention_stream_cache_gather", args + (None,))


def _refusals():
    nan, inf = float("nan"), float("inf")
    out = []
    # the options of the two forward entries: gain, head counts, ids
    for make in (_fwd, _varlen):
        for o, what in ((_opts(bias_gain=nan), "gain"), (_opts(bias_gain=-1.0), "gain"), (_opts(bias_gain=inf), "gain"),
                        (_opts(bias_gain=3.4e38), "out of range"), (_opts(n_same=-1, n_other=1, speakers=P16), ">= 0"),
                        (_opts(n_same=1, n_other=-1, speakers=P16), ">= 0"), (_opts(n_same=H, n_other=1, speakers=P16), "exceeds"),
                        (_opts(n_same=256, speakers=P16), "exceeds"), (_opts(n_same=1, n_other=1), "need speakers"),
                        (_opts(n_other=1), "need speakers")):
            out.append((make(o), what))
    # the long-dialogue entries' own arguments, forward and backward
    for bwd in (False, True):
        out += [(_varlen(None, bwd, L=513), "L <= 512"), (_varlen(None, bwd, L=0), "L <= 512"), (_varlen(None, bwd, B=0), "L <= 512"),
                (_varlen(None, bwd, cu=P16), "exactly one"), (_varlen(None, bwd, key_pad=None), "exactly one"),
                (_varlen(None, bwd, cu=P16, key_pad=None, T=0), "T >= 1"), (_varlen(None, bwd, B=4096, L=512), "2^32")]
    # the two stream entries: shapes, pointers, paging, options
    for chunk in (False, True):
        new = "[S][T]" if chunk else "[S]"
        out += [(_stream(None, chunk, S=0), "required"), (_stream(None, chunk, H=0), "required"), (_stream(None, chunk, hd=129), "required"),
                (_stream(None, chunk, C=513), "required"), (_stream(None, chunk, C=0), "required"),
                (_stream(None, chunk, q=None), "NULL"), (_stream(None, chunk, count=None), "NULL"), (_stream(None, chunk, second=None), "NULL"),
                (_stream(None, chunk, out=None), "NULL"), (_stream(None, chunk, kc=None), "NULL"),
                (_stream(None, chunk, ld=E - 1), "leading dimension"), (_stream(None, chunk, kc=P4), "16-byte aligned"),
                (_stream(None, chunk, vc=P4), "16-byte aligned"),
                (_stream(_paged(page_rows=8), chunk), "page_rows"), (_stream(_paged(n_pages=0), chunk), "n_pages"),
                (_stream(_paged(table_cols=2), chunk), "table must be int32"), (_stream(_paged(), chunk, C=17), "table must be int32"),
                (_stream(_paged(), chunk, kc=P4), "pools must be 16-byte aligned"), (_stream(_paged(table=P1), chunk), "4-byte aligned"),
                (_stream(_paged(), chunk, vc=None), "NULL"), (_stream(_paged(), chunk, hd=129), "required"),
                (_stream(_sopts(bias_gain=nan), chunk), "gain"), (_stream(_sopts(bias_gain=-0.5), chunk), "gain"),
                (_stream(_sopts(bias_gain=3.4e38), chunk), "out of range"),
                (_stream(_sopts(n_same=-1, spk_cache=P16, spk_new=P16), chunk), ">= 0"),
                (_stream(_sopts(n_same=H, n_other=1, spk_cache=P16, spk_new=P16), chunk), "exceeds"),
                (_stream(_sopts(n_same=1, n_other=1, spk_cache=P16), chunk), "speakers (uint8 " + new + ")"),
                (_stream(_sopts(n_same=1, n_other=1, spk_new=P16), chunk), "cached speakers"),
                (_stream(_paged(n_same=1, spk_new=P16), chunk), "cached speakers")]
    out += [(_stream(_sopts(weights=P1)), "weights"), (_stream(_paged(weights=P1)), "weights"),
            (_stream(_sopts(weights=P16), True), "weights must be NULL"), (_stream(_paged(weights=P16), True), "weights must be NULL"),
            (_stream(None, True, T=0), "T <= 64"), (_stream(None, True, T=65), "T <= 64"), (_stream(_paged(), True, T=65), "T <= 64")]
    # snapshot / restore: dense and paged through the same two entries
    for scatter in (False, True):
        out += [(_cache(scatter, S=0), "required"), (_cache(scatter, C=513), "required"), (_cache(scatter, kc=None), "NULL"),
                (_cache(scatter, kc=P4), "16-byte aligned"), (_cache(scatter, n=-1), ">= 0"), (_cache(scatter, elems=-1), ">= 0"),
                (_cache(scatter, slots=None), "NULL"), (_cache(scatter, packed=P4), "packed buffer"), (_cache(scatter, offsets=P4), "row_offsets"),
                (_cache(scatter, table=P4, table_cols=1, n_pages=2, page_rows=8), "page_rows"),
                (_cache(scatter, table=P4, table_cols=2, n_pages=2, page_rows=R), "table must be int32"),
                (_cache(scatter, table=P4, table_cols=1, n_pages=0, page_rows=R), "n_pages"),
                (_cache(scatter, table=P1, table_cols=1, n_pages=2, page_rows=R), "4-byte aligned"),
                (_cache(scatter, table=P4, table_cols=1, n_pages=2, page_rows=R, vc=P4), "pools must be 16-byte aligned")]
    out.append((_cache(True, count=None), "NULL"))
    return out


REFUSALS = _refusals()


@pytest.mark.parametrize("call,what", REFUSALS, ids=[f"{i:03d}-{c[0][4:]}-{w.split()[0]}" for i, (c, w) in enumerate(REFUSALS)])
def test_refused_before_any_launch(call, what):
    name, args = call
    lib = runtime.lib()
    code = getattr(lib, name)(*args)
    msg = lib.m2f_last_error().decode()
    assert code != 0, f"{name} accepted a launch it must refuse ({what})"
    assert msg.startswith(name + ": ") and what in msg, msg


def test_every_entry_and_refusal_kind_is_covered():
    names = {c[0] for c, _ in REFUSALS}
    assert names == {"m2f_attention_fwd", "m2f_attention_varlen_fwd", "m2f_attention_varlen_bwd", "m2f_attention_stream",
                     "m2f_attention_stream_chunk", "m2f_attention_stream_cache_gather", "m2f_attention_stream_cache_scatter"}
    # (m2f_attention_bwd has no argument of its own to refuse: its shape limits are the launcher's, behind the entry)
    assert "m2f_attention_bwd" in runtime.SIGNATURES


@pytest.mark.parametrize("which,mirror,c_name", [(0, runtime.AttnOptsC, "m2f_attn_opts"), (1, runtime.AttnStreamOptsC, "m2f_attn_stream_opts")])
def test_structures_have_the_layout_the_library_was_compiled_with(which, mirror, c_name):
    lib = runtime.lib()
    n = lib.m2f_attention_opts_layout(which, None, 0)
    assert n == 1 + len(mirror._fields_), f"{c_name}: the C struct has {n - 1} fields, the Structure {len(mirror._fields_)}"
    buf = (ctypes.c_int * n)()
    assert lib.m2f_attention_opts_layout(which, buf, n) == n
    assert buf[0] == ctypes.sizeof(mirror), (c_name, buf[0], ctypes.sizeof(mirror))
    assert list(buf[1:]) == [getattr(mirror, f).offset for f, _ in mirror._fields_], c_name
    # ... and the header declares the fields under the Structure's names, in its order
    header = open(runtime.HEADER_PATH).read()
    struct = header[header.index("typedef struct " + c_name + " {"):header.index("} " + c_name + ";")]
    code = " ".join(line.split("/*")[0] for line in struct.split("\n"))
    at = [code.index(f) for f, _ in mirror._fields_]
    assert at == sorted(at), (c_name, at)
    assert lib.m2f_attention_opts_layout(2, None, 0) < 0


def test_no_option_initialiser_and_the_retired_forms():
    header = open(runtime.HEADER_PATH).read()
    assert "#define M2F_ATTN_OPTS_NONE {-1, -1, 0.f, 0, 0, NULL}" in header
    # paging and the weights rows are fields now: no entry carries them in its name
    for base, suffixes in (("m2f_attention_stream", ("_paged", "_weights", "_weights_paged")), ("m2f_attention_stream_chunk", ("_paged",)),
                           ("m2f_attention_stream_cache_gather", ("_paged",)), ("m2f_attention_stream_cache_scatter", ("_paged",))):
        for suffix in suffixes:
            old = base + suffix
            assert old not in runtime.SIGNATURES and (old + "(") not in header and not hasattr(runtime.lib(), old), old
