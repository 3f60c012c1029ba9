"""JSON schemas written out as regular expressions of dflash_amd.regex's subset.

json_schema_regex(schema) -> the pattern whose full matches are the JSON texts the schema admits, with
whitespace_pattern between the structural characters.  Properties come in declared order; optional ones may be absent;
additionalProperties: false is implied.  A keyword outside the supported list is refused by name: a constraint that is
silently ignored is worse than a refusal.
"""
from __future__ import annotations

import json

_META = "\\.[]{}()*+?|^$-/"
STRING_INNER = r'([^"\\\x00-\x1f]|\\["\\/bfnrt]|\\u[0-9a-fA-F]{4})'
STRING = '"' + STRING_INNER + '*"'
INTEGER = r"-?(0|[1-9][0-9]*)"
NUMBER = INTEGER + r"(\.[0-9]+)?([eE][+-]?[0-9]+)?"
BOOLEAN = r"(true|false)"
NULL = r"null"

# annotations: they constrain nothing, so they are read over
_ANNOTATIONS = {"title", "description", "$schema", "$id", "$defs", "definitions"}
_COMMON = {"type", "enum", "const", "anyOf", "oneOf", "$ref"} | _ANNOTATIONS
_BY_TYPE = {
    "string": {"minLength", "maxLength", "pattern"},
    "array": {"items", "minItems", "maxItems"},
    "object": {"properties", "required", "additionalProperties"},
    "integer": set(), "number": set(), "boolean": set(), "null": set(),
}


def _escape(text: str) -> str:
    out = []
    for ch in text:
        if ch in _META:
            out.append("\\" + ch)
        elif ord(ch) < 32 or ord(ch) == 127:
            out.append(f"\\x{ord(ch):02x}")
        else:
            out.append(ch)
    return "".join(out)


def _literal(value) -> str:
    return _escape(json.dumps(value, ensure_ascii=False, separators=(",", ":")))


def _is_type(v, t: str) -> bool:
    if t == "null":
        return v is None
    if t == "boolean":
        return isinstance(v, bool)
    if t in ("integer", "number"):
        return not isinstance(v, bool) and (isinstance(v, int) or (isinstance(v, float) and (t == "number" or v == int(v))))
    return isinstance(v, {"string": str, "array": list, "object": dict}[t])


def _count(schema, key, where):
    v = schema.get(key)
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise ValueError(f"dflash_amd: json_schema: {where}{key} = {v!r} is no count")
    return v


class _Writer:
    def __init__(self, root, ws):
        self.root, self.ws = root, ws
        self.open_refs = []

    def resolve(self, ref, where):
        if not isinstance(ref, str) or not (ref.startswith("#/$defs/") or ref.startswith("#/definitions/")):
            raise ValueError(f"dflash_amd: json_schema: {where}$ref {ref!r}: only local #/$defs/NAME or #/definitions/NAME")
        _, table, name = ref.split("/", 2)
        try:
            return self.root[table][name]
        except (KeyError, TypeError):
            raise ValueError(f"dflash_amd: json_schema: {where}$ref {ref!r} names nothing") from None

    def write(self, s, where="") -> str:
        if not isinstance(s, dict):
            raise ValueError(f"dflash_amd: json_schema: {where or 'the schema'} is not an object")
        if "$ref" in s:
            extra = sorted(set(s) - {"$ref"} - _ANNOTATIONS)
            if extra:
                raise ValueError(f"dflash_amd: json_schema: {where}{extra[0]} beside $ref is not supported")
            ref = s["$ref"]
            if ref in self.open_refs:
                raise ValueError(f"dflash_amd: json_schema: {where}$ref {ref!r} is recursive: no regular expression")
            self.open_refs.append(ref)
            try:
                return self.write(self.resolve(ref, where), where)
            finally:
                self.open_refs.pop()
        types = s.get("type")
        types = [types] if isinstance(types, str) else types
        if types is not None and (not isinstance(types, list) or not types or any(t not in _BY_TYPE for t in types)):
            raise ValueError(f"dflash_amd: json_schema: {where}type {s.get('type')!r} is not supported")
        allowed = set(_COMMON)
        for t in types or ():
            allowed |= _BY_TYPE[t]
        for key in s:
            if key not in allowed:
                known = any(key in v for v in _BY_TYPE.values())
                raise ValueError(f"dflash_amd: json_schema: {where}keyword {key!r} is not supported"
                                 + (f" for type {s.get('type')!r}" if known else ""))
        kinds = [k for k in ("enum", "const", "anyOf", "oneOf") if k in s]
        if len(kinds) + (types is not None) > 1:
            both = kinds + (["type"] if types is not None else [])
            if not (types is not None and kinds in (["enum"], ["const"])):
                raise ValueError(f"dflash_amd: json_schema: {where}{both[0]} beside {both[1]} is not supported")
        if "const" in s or "enum" in s:
            values = [s["const"]] if "const" in s else s["enum"]
            if not isinstance(values, list) or not values:
                raise ValueError(f"dflash_amd: json_schema: {where}enum is a non-empty list")
            if types is not None:   # `type` beside them still constrains: the values of another type drop out
                values = [v for v in values if any(_is_type(v, t) for t in types)]
                if not values:
                    raise ValueError(f"dflash_amd: json_schema: {where}no enum / const value has type {s['type']!r}")
            return "(" + "|".join(_literal(v) for v in values) + ")"
        for k in ("anyOf", "oneOf"):
            if k in s:
                if not isinstance(s[k], list) or not s[k]:
                    raise ValueError(f"dflash_amd: json_schema: {where}{k} is a non-empty list")
                return "(" + "|".join(self.write(a, f"{where}{k}[{i}].") for i, a in enumerate(s[k])) + ")"
        if types is None:
            raise ValueError(f"dflash_amd: json_schema: {where or 'the schema '}has no type, enum, const, anyOf, oneOf or $ref")
        arms = [getattr(self, "w_" + t)(s, where) for t in types]
        return arms[0] if len(arms) == 1 else "(" + "|".join(arms) + ")"

    def w_integer(self, s, where):
        return INTEGER

    def w_number(self, s, where):
        return NUMBER

    def w_boolean(self, s, where):
        return BOOLEAN

    def w_null(self, s, where):
        return NULL

    def w_string(self, s, where):
        lo, hi = _count(s, "minLength", where), _count(s, "maxLength", where)
        if "pattern" in s:
            if lo is not None or hi is not None:
                raise ValueError(f"dflash_amd: json_schema: {where}minLength / maxLength beside pattern is not supported")
            p = s["pattern"]
            if not isinstance(p, str):
                raise ValueError(f"dflash_amd: json_schema: {where}pattern is a string")
            p = p[1:] if p.startswith("^") else p
            p = p[:-1] if p.endswith("$") and not p.endswith("\\$") else p
            return '"(' + p + ')"'
        if lo is None and hi is None:
            return STRING
        if hi is not None and hi < (lo or 0):
            raise ValueError(f"dflash_amd: json_schema: {where}maxLength below minLength")
        return '"' + STRING_INNER + "{" + str(lo or 0) + "," + ("" if hi is None else str(hi)) + '}"'

    def w_array(self, s, where):
        if "items" not in s:
            raise ValueError(f"dflash_amd: json_schema: {where}an array without items (any value) is not supported")
        lo, hi = _count(s, "minItems", where) or 0, _count(s, "maxItems", where)
        if hi is not None and hi < lo:
            raise ValueError(f"dflash_amd: json_schema: {where}maxItems below minItems")
        ws = self.ws
        if hi == 0:
            return r"\[" + ws + r"\]"
        item = self.write(s["items"], where + "items.")
        more = "(" + ws + "," + ws + item + "){" + str(max(lo - 1, 0)) + "," + ("" if hi is None else str(hi - 1)) + "}"
        body = item + more
        if lo == 0:
            body = "(" + body + ")?"
        return r"\[" + ws + body + ws + r"\]"

    def w_object(self, s, where):
        ws = self.ws
        if s.get("additionalProperties", False) is not False:
            raise ValueError(f"dflash_amd: json_schema: {where}additionalProperties other than false is not supported")
        props = s.get("properties", {})
        if not isinstance(props, dict):
            raise ValueError(f"dflash_amd: json_schema: {where}properties is an object")
        required = s.get("required", [])
        if not isinstance(required, list) or any(r not in props for r in required):
            raise ValueError(f"dflash_amd: json_schema: {where}required names a property that is not declared")
        names = list(props)
        pats = [_literal(n) + ws + ":" + ws + self.write(props[n], f"{where}{n}.") for n in names]
        need = [n in required for n in names]
        comma = ws + "," + ws
        if any(need):
            last = max(i for i, r in enumerate(need) if r)
            body = ""
            for i in range(last):
                body += pats[i] + comma if need[i] else "(" + pats[i] + comma + ")?"
            body += pats[last]
            for i in range(last + 1, len(names)):
                body += "(" + comma + pats[i] + ")?"
        elif names:
            arms = []
            for i in range(len(names)):     # property i is the first one present
                arms.append(pats[i] + "".join("(" + comma + pats[j] + ")?" for j in range(i + 1, len(names))))
            body = "(" + "|".join(arms) + ")?"
        else:
            body = ""
        return r"\{" + ws + body + ws + r"\}"


def json_schema_regex(schema: dict, *, whitespace_pattern: str = "[ ]?") -> str:
    """The regular expression of the JSON texts `schema` admits.  Supported: type (string, integer, number, boolean,
    null, array, object, or a list of them), enum, const, minLength / maxLength, pattern, items, minItems / maxItems,
    properties (declared order), required, additionalProperties: false (implied), anyOf / oneOf (alternation), local
    $ref into #/$defs or #/definitions (not recursive); title, description, $schema and $id are read over.  Anything else
    is a ValueError naming the keyword."""
    if not isinstance(schema, dict):
        raise ValueError("dflash_amd: json_schema: the schema is a dict")
    return _Writer(schema, whitespace_pattern).write(schema)
