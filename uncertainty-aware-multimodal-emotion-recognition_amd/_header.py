"""Parser of include/mmdeer.h: the header is the one statement of the C ABI, and the ctypes binding (_lib.py) is derived from it.
Its companions include/mmdeer_video.h (the temporal video encoder's operators), include/mmdeer_frames.h (the Conv2d backbone on
frames), include/mmdeer_frames_bwd.h (its backward), include/mmdeer_routes.h (the layer chains' route queries), include/mmdeer_bert.h (the BERT trunk's forward operators), include/mmdeer_bert_bwd.h (their backward) include/mmdeer_bert_drop.h (both with the trunk's dropout inside) include/mmdeer_optim.h (clip + AdamW over any list of tensors) include/mmdeer_graph.h (device step counters for HIP-graph replays) include/mmdeer_drop_dev.h (the same counter for the three by-value dropout entries of mmdeer.h) and include/mmdeer_seqlen.h (the audio encoder's recurrence and pool with per-sample lengths) are written in the same grammar and parsed here too.

The header is regular: ``#define MMDEER_X <integer>``, ``typedef struct [tag] { fields } name;`` and ``type mmdeer_x(params);``.
Anything else raises a HeaderError that quotes the text: no declaration and no preprocessor line is skipped (the include guard,
the two #include lines and the ``#ifdef __cplusplus`` pair are the only other directives accepted; a conditional branch, a
function-like macro or a #define outside the MMDEER_ prefix raises).
"""
from __future__ import annotations

import ctypes as C
import re

from .build import BERT_BWD_HEADER_PATH, BERT_DROP_HEADER_PATH, BERT_HEADER_PATH, DROP_DEV_HEADER_PATH, FRAMES_BWD_HEADER_PATH, FRAMES_HEADER_PATH, GRAPH_HEADER_PATH, HEADER_PATH, OPTIM_HEADER_PATH, ROUTES_HEADER_PATH, SEQLEN_HEADER_PATH, VIDEO_HEADER_PATH

SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "float": C.c_float, "double": C.c_double, "uint64_t": C.c_uint64,
           "unsigned long long": C.c_uint64, "long long": C.c_longlong, "int64_t": C.c_int64, "size_t": C.c_size_t}
POINTEES = {"void", "char", "unsigned char"}       # base types that occur behind a star only

_DEFINE = re.compile(r"define\s+MMDEER_(\w+)\s+(\S.*)")
_DIRECTIVE = re.compile(r"include\s*<\w+\.h>|ifndef\s+MMDEER_(VIDEO_|FRAMES_|FRAMES_BWD_|ROUTES_|BERT_|BERT_BWD_|BERT_DROP_|OPTIM_|GRAPH_|DROP_DEV_|SEQLEN_)?H_|define\s+MMDEER_(VIDEO_|FRAMES_|FRAMES_BWD_|ROUTES_|BERT_|BERT_BWD_|BERT_DROP_|OPTIM_|GRAPH_|DROP_DEV_|SEQLEN_)?H_|ifdef\s+__cplusplus|endif")    # carry no declaration
_OPAQUE = re.compile(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;\s*")
_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;\s*")
_PROTO = re.compile(r"([\w\s*]+?)\b(mmdeer_\w+)\s*\(([^(){};]*)\)\s*;\s*")
_DECL = re.compile(r"([\w\s*]*?)(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*$")


class HeaderError(ValueError):
    """A declaration of the header that this parser cannot account for."""


def _integer(expr: str, consts: dict) -> int:
    """A product of integer literals and earlier constants, parentheses around it allowed."""
    value = 1
    for factor in expr.strip().strip("()").split("*"):
        factor = factor.strip().removeprefix("MMDEER_")
        if not re.fullmatch(r"\d+", factor) and factor not in consts:
            raise HeaderError(f"mmdeer.h: not an integer expression: {expr!r}")
        value *= consts[factor] if factor in consts else int(factor)
    return value


def parse(text: str, names: dict, overrides: dict):
    """-> (constants {NAME: int} without the MMDEER_ prefix, classes {C struct name: ctypes.Structure subclass},
    symbols [(name, restype, argtypes)]).  ``names``: C struct name -> Python class name.  ``overrides``: (C struct name, field) ->
    element ctypes type of a pointer field that stays POINTER(element) instead of c_void_p (the host assigns ctypes arrays to it)."""
    consts, classes, symbols, opaque, used = {}, {}, [], set(), set()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    for line in re.findall(r"^[ \t]*#[ \t]*(.*?)[ \t]*$", text, flags=re.M):
        if m := _DEFINE.fullmatch(line):
            consts[m.group(1)] = _integer(m.group(2), consts)
        elif not _DIRECTIVE.fullmatch(line):
            raise HeaderError(f"mmdeer.h: unsupported preprocessor line {'#' + line!r}")
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}\s*$', r"\1", text, flags=re.S)       # the block's braces; its content stays

    def ctype(spec: str, nptr: int, what: str):
        words = spec.split()
        base = " ".join(w for w in words if w != "const")
        if nptr == 0 and base in SCALARS:
            return SCALARS[base]
        if nptr == 0 and base in classes:
            return classes[base]
        if nptr == 1 and base == "char" and "const" in words:
            return C.c_char_p
        if nptr == 1 and base in classes:
            return C.POINTER(classes[base])
        if nptr >= 1 and (base in SCALARS or base in POINTEES or base in opaque or base in classes):
            return C.c_void_p
        raise HeaderError(f"mmdeer.h: unknown type {spec.strip() + '*' * nptr!r} in {what!r}")

    def declarator(decl: str, spec, what: str, owner=None):
        """'const float* g_out[7]' -> ('g_out', c_void_p * 7, 'const float'); a declarator behind a comma takes ``spec`` from the first."""
        m = _DECL.match(decl.strip())
        has_type = bool(m and m.group(1).replace("*", "").strip())
        if not m or (spec is None and not has_type) or (spec is not None and has_type):   # the first declarator names the type,
            raise HeaderError(f"mmdeer.h: cannot parse {decl.strip()!r} in {what!r}")      # one behind a comma must not
        spec = m.group(1).replace("*", " ") if spec is None else spec
        name, nptr = m.group(2), m.group(1).count("*")
        t = ctype(spec, nptr, what)
        if (owner, name) in overrides:
            if nptr < 1 or ctype(spec, nptr - 1, what) is not overrides[owner, name]:
                raise HeaderError(f"mmdeer.h: override of {owner}.{name} does not match {decl.strip()!r}")
            t = C.POINTER(overrides[owner, name])
            used.add((owner, name))
        if m.group(3):
            t = t * _integer(m.group(3), consts)
        return name, t, spec

    text = text.strip()
    pos = 0
    while pos < len(text):
        if m := _OPAQUE.match(text, pos):
            if m.group(1) != m.group(2):
                raise HeaderError(f"mmdeer.h: unsupported typedef {m.group(0).strip()!r}")
            opaque.add(m.group(2))
        elif m := _STRUCT.match(text, pos):
            body, cname = m.group(1), m.group(2)
            fields = []
            for stmt in filter(str.strip, body.split(";")):
                spec = None
                for decl in stmt.split(","):
                    name, t, spec = declarator(decl, spec, stmt.strip(), cname)
                    fields.append((name, t))
            if cname not in names:
                raise HeaderError(f"mmdeer.h: struct {cname} has no Python class name")
            classes[cname] = type(names[cname], (C.Structure,), {"_fields_": fields, "__doc__": f"{cname} (include/mmdeer.h)."})
        elif m := _PROTO.match(text, pos):
            what = " ".join(m.group(0).split())
            params = [] if m.group(3).strip() == "void" else m.group(3).split(",")
            ret = m.group(1)
            restype = None if ret.split() == ["void"] else ctype(ret.replace("*", " "), ret.count("*"), what)
            symbols.append((m.group(2), restype, [declarator(p, None, what)[1] for p in params]))
        else:
            raise HeaderError(f"mmdeer.h: cannot parse the declaration {text[pos:].split(';')[0].strip()[:200]!r}")
        pos = m.end()
    if set(overrides) - used:
        raise HeaderError(f"mmdeer.h: override of a field that does not exist: {sorted(set(overrides) - used)}")
    return consts, classes, symbols


def read(path: str = HEADER_PATH):
    with open(path) as f:
        return f.read()
