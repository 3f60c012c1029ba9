"""dflash_amd.json_schema: seeded random walks of the compiled automaton give texts json.loads
accepts and a small checker (below: jsonschema may be absent) finds valid; hand-written invalid documents are rejected;
unsupported keywords and recursive references are refused by name.  And Vocabulary.from_tokenizer on a stub."""
import json

import numpy as np
import pytest

import grammar_lift_common as C
from dflash_amd import Vocabulary, compile_grammar, compile_regex, json_schema_regex

USER = {"type": "object", "required": ["name"], "properties": {
    "name": {"type": "string", "minLength": 1, "maxLength": 6}, "age": {"type": "integer"}}}
SCHEMAS = {
    "flat": {"type": "object", "required": ["id", "name"], "properties": {
        "id": {"type": "integer"}, "name": {"type": "string"}, "score": {"type": "number"}, "ok": {"type": "boolean"},
        "none": {"type": "null"}}},
    "all_optional": {"type": "object", "properties": {"a": {"type": "integer"}, "b": {"type": "boolean"},
                                                      "c": {"type": "null"}}},
    "optional_around_required": {"type": "object", "required": ["m"], "properties": {
        "a": {"type": "boolean"}, "b": {"type": "integer"}, "m": {"type": "null"}, "y": {"type": "boolean"},
        "z": {"type": "integer"}}},
    "nested": {"type": "object", "required": ["user"], "properties": {
        "user": USER, "tags": {"type": "array", "items": {"type": "string", "maxLength": 3}}}},
    "bounded_array": {"type": "array", "items": {"type": "integer"}, "minItems": 2, "maxItems": 4},
    "array_up_to": {"type": "array", "items": {"type": "boolean"}, "maxItems": 2},
    "empty_array": {"type": "array", "items": {"type": "boolean"}, "maxItems": 0},
    "array_of_objects": {"type": "array", "items": USER, "minItems": 1, "maxItems": 2},
    "enum": {"enum": ["red", "a\"b", 3, 2.5, True, None, {"k": [1, 2]}]},
    "const": {"type": "object", "required": ["v"], "properties": {"v": {"const": "é/\\"}}},
    "any_of": {"anyOf": [{"type": "integer"}, {"type": "string", "maxLength": 2}, {"type": "array", "items": {"type": "null"}}]},
    "one_of": {"type": "object", "required": ["x"], "properties": {"x": {"oneOf": [{"type": "boolean"}, {"const": 0}]}}},
    "ref": {"type": "object", "required": ["a"], "properties": {"a": {"$ref": "#/$defs/user"}, "b": {"$ref": "#/definitions/n"}},
            "$defs": {"user": USER}, "definitions": {"n": {"type": "number"}}, "title": "T", "description": "d"},
    "pattern": {"type": "object", "required": ["mail"], "properties": {
        "mail": {"type": "string", "pattern": "^[a-z]{1,4}@[a-z]{1,4}\\.(com|org)$"}}},
    "type_list": {"type": ["integer", "null"]},
    "no_properties": {"type": "object"},
}


def valid(v, s, root):
    """A small JSON-schema checker over the supported keywords (additionalProperties: false implied, declared order)."""
    if "$ref" in s:
        _, table, name = s["$ref"].split("/")
        return valid(v, root[table][name], root)
    if "const" in s:
        return v == s["const"] and type(v) is type(s["const"])
    if "enum" in s:
        return any(v == e and type(v) is type(e) for e in s["enum"])
    for k in ("anyOf", "oneOf"):
        if k in s:
            return any(valid(v, a, root) for a in s[k])
    types = s["type"] if isinstance(s["type"], list) else [s["type"]]
    return any(valid_as(v, t, s, root) for t in types)


def valid_as(v, t, s, root):
    if t == "null":
        return v is None
    if t == "boolean":
        return isinstance(v, bool)
    if t == "integer":
        return isinstance(v, int) and not isinstance(v, bool)
    if t == "number":
        return isinstance(v, (int, float)) and not isinstance(v, bool)
    if t == "string":
        if not isinstance(v, str) or not s.get("minLength", 0) <= len(v) <= s.get("maxLength", 1 << 30):
            return False
        import re
        return "pattern" not in s or re.fullmatch(s["pattern"].strip("^$"), v) is not None
    if t == "array":
        return (isinstance(v, list) and s.get("minItems", 0) <= len(v) <= s.get("maxItems", 1 << 30)
                and all(valid(x, s["items"], root) for x in v))
    props = s.get("properties", {})
    if not isinstance(v, dict) or any(k not in props for k in v) or any(r not in v for r in s.get("required", [])):
        return False
    order = [k for k in props if k in v]
    return list(v) == order and all(valid(x, props[k], root) for k, x in v.items())


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_random_walks_are_valid_documents(name):
    schema = SCHEMAS[name]
    dfa = compile_regex(json_schema_regex(schema))
    rng = np.random.default_rng(len(name))
    seen = set()
    for _ in range(40):
        text = C.accepted_text(dfa, rng, max_len=120).decode("utf-8")
        doc = json.loads(text)
        assert valid(doc, schema, schema), (name, text)
        seen.add(text)
    assert len(seen) > 1 or name in ("const", "empty_array", "no_properties")      # (those three admit 1..4 texts)


def test_optional_properties_in_every_subset():
    """Every subset of the optional properties, in declared order, with the commas right; nothing else."""
    import itertools
    for name in ("all_optional", "optional_around_required"):
        schema = SCHEMAS[name]
        dfa = compile_regex(json_schema_regex(schema))
        values = {"boolean": "true", "integer": "-7", "null": "null"}
        props = list(schema["properties"])
        req = schema.get("required", [])
        for keep in itertools.product([False, True], repeat=len(props)):
            chosen = [p for p, k in zip(props, keep) if k]
            body = ",".join(f'"{p}":{values[schema["properties"][p]["type"]]}' for p in chosen)
            ok = all(r in chosen for r in req)
            assert dfa.matches(("{" + body + "}").encode()) == ok, (name, body)
            assert dfa.matches(("{ " + body.replace(",", " , ").replace(":", " : ") + " }").encode()) == ok
            if body:
                assert not dfa.matches(("{" + body + ",}").encode()) and not dfa.matches(("{," + body + "}").encode())
            if len(chosen) > 1:
                swapped = ",".join(reversed(body.split(",")))
                assert not dfa.matches(("{" + swapped + "}").encode()), swapped


INVALID = [
    ("flat", '{"id":1}'),                                        # a missing required key
    ("flat", '{"name":"x","id":1}'),                             # the declared order
    ("flat", '{"id":"1","name":"x"}'),                           # a wrong type
    ("flat", '{"id":1.5,"name":"x"}'),
    ("flat", '{"id":1,"name":"x",}'),                            # a trailing comma
    ("flat", '{"id":1,"name":"x","extra":1}'),                   # an extra key
    ("flat", '{"id":01,"name":"x"}'),                            # a leading zero
    ("flat", '{"id":1,"name":"a\nb"}'),                          # a raw control character in a string
    ("flat", '{"id":1,"name":"a\\qb"}'),                         # an escape JSON does not have
    ("flat", '{"id":1,"name":"x"'),
    ("nested", '{"user":{"age":3}}'), ("nested", '{"user":{"name":""}}'), ("nested", '{"user":{"name":"abcdefg"}}'),
    ("nested", '{"user":{"name":"a"},"tags":["abcd"]}'), ("nested", '{"user":{"name":"a"},"tags":["a",]}'),
    ("bounded_array", "[1]"), ("bounded_array", "[1,2,3,4,5]"), ("bounded_array", "[1,,2]"), ("bounded_array", "[1,true]"),
    ("empty_array", "[true]"), ("enum", '"blue"'), ("enum", "3.0"), ("const", '{"v":"e"}'), ("any_of", "true"),
    ("any_of", '"abc"'), ("one_of", '{"x":1}'), ("pattern", '{"mail":"a@b.net"}'), ("type_list", "1.5"),
    ("no_properties", '{"a":1}'),
]


@pytest.mark.parametrize("name,text", INVALID, ids=[f"{n}-{i}" for i, (n, _) in enumerate(INVALID)])
def test_invalid_documents_are_rejected(name, text):
    assert not compile_regex(json_schema_regex(SCHEMAS[name])).matches(text.encode("utf-8"))


VALID = [("flat", '{"id":-12,"name":"a\\"b\\u00e9\\n é","score":-1.5e+3,"ok":false,"none":null}'),
         ("flat", '{ "id" : 0 , "name" : "" }'), ("enum", '{"k":[1,2]}'), ("enum", '"a\\"b"'), ("const", '{"v":"é/\\\\"}'),
         ("empty_array", "[ ]"), ("no_properties", "{}"), ("pattern", '{"mail":"ab@cd.org"}')]


@pytest.mark.parametrize("name,text", VALID, ids=[f"{n}-{i}" for i, (n, _) in enumerate(VALID)])
def test_hand_written_valid_documents_are_accepted(name, text):
    assert valid(json.loads(text), SCHEMAS[name], SCHEMAS[name])
    assert compile_regex(json_schema_regex(SCHEMAS[name])).matches(text.encode("utf-8"))


@pytest.mark.parametrize("schema,name", [
    ({"type": "integer", "minimum": 0}, "minimum"), ({"type": "string", "format": "date"}, "format"),
    ({"type": "object", "properties": {}, "patternProperties": {}}, "patternProperties"),
    ({"type": "object", "additionalProperties": True}, "additionalProperties"),
    ({"type": "array", "items": {"type": "null"}, "uniqueItems": True}, "uniqueItems"),
    ({"type": "array", "prefixItems": []}, "prefixItems"), ({"allOf": [{"type": "null"}]}, "allOf"),
    ({"not": {"type": "null"}}, "not"), ({"type": "integer", "minLength": 2}, "minLength"),
    ({"type": "object", "properties": {"a": {"type": "number", "multipleOf": 2}}}, "multipleOf"),
    ({"type": "array"}, "items"), ({"type": "date"}, "date"), ({}, "no type"),
    ({"$ref": "http://example.com/x"}, "only local"), ({"$ref": "#/$defs/missing", "$defs": {}}, "names nothing"),
    ({"type": "object", "properties": {"a": {"type": "null"}}, "required": ["b"]}, "required"),
])
def test_unsupported_keywords_are_refused_by_name(schema, name):
    with pytest.raises(ValueError, match="json_schema: .*" + name):
        json_schema_regex(schema)


def test_recursive_ref_is_refused():
    tree = {"$ref": "#/$defs/node", "$defs": {"node": {"type": "object", "properties": {
        "kids": {"type": "array", "items": {"$ref": "#/$defs/node"}}}}}}
    with pytest.raises(ValueError, match="recursive"):
        json_schema_regex(tree)


def test_whitespace_pattern_and_compile_grammar():
    tight = compile_regex(json_schema_regex(SCHEMAS["bounded_array"], whitespace_pattern=""))
    assert tight.matches(b"[1,2]") and not tight.matches(b"[1, 2]")
    voc = Vocabulary([bytes([b]) for b in range(256)], eos_ids=(0,))
    g = compile_grammar(json_schema=SCHEMAS["bounded_array"], vocabulary=voc)
    assert g.num_states == compile_regex(json_schema_regex(SCHEMAS["bounded_array"])).num_states and g.vocab_size == 256
    assert compile_grammar(regex="ab*", vocabulary=voc).num_states == 2
    for kw in (dict(), dict(regex="a", json_schema={"type": "null"})):
        with pytest.raises(ValueError, match="exactly one"):
            compile_grammar(vocabulary=voc, **kw)


class StubTokenizer:
    """What Vocabulary.from_tokenizer reads of a byte-level BPE tokenizer."""
    eos_token_id = 6

    def __init__(self, vocab, added):
        self.vocab, self.added = vocab, added

    def get_vocab(self):
        return dict(self.vocab)

    def get_added_vocab(self):
        return dict(self.added)


def test_vocabulary_from_a_byte_level_tokenizer():
    from dflash_amd.grammar import _bytes_to_unicode
    table = _bytes_to_unicode()
    assert len(set(table.values())) == 256 and table[ord("a")] == "a" and table[ord(" ")] == "Ġ" and table[10] == "Ċ"
    spell = lambda b: "".join(table[x] for x in b)                                     # noqa: E731
    words = [b"a", b" the", "é".encode(), b"\n\n", b"\xff\x00", b"{\""]
    vocab = {spell(w): i for i, w in enumerate(words)}
    vocab["<|endoftext|>"] = 6
    voc = Vocabulary.from_tokenizer(StubTokenizer(vocab, {"<|endoftext|>": 6}), vocab_size=16)
    assert len(voc) == 16 and voc.token_bytes[:6] == words
    assert voc.token_bytes[6] == b"" and all(t == b"" for t in voc.token_bytes[7:])    # the added token, the padding
    assert voc.eos_ids == (6,)
    data, off = voc.flat()
    assert data.dtype == np.uint8 and off.dtype == np.int32 and off.shape == (17,) and off[-1] == data.size
    assert bytes(data[off[1]:off[2]]) == b" the"
    assert len(Vocabulary.from_tokenizer(StubTokenizer(vocab, {"<|endoftext|>": 6}))) == 7
    with pytest.raises(ValueError, match="not byte-level BPE"):                        # a sentencepiece-style piece
        Vocabulary.from_tokenizer(StubTokenizer({"▁the": 0, "a": 1}, {}))
    with pytest.raises(ValueError, match="vocab_size 4 below"):
        Vocabulary.from_tokenizer(StubTokenizer(vocab, {"<|endoftext|>": 6}), vocab_size=4)
    with pytest.raises(ValueError, match="get_vocab"):
        Vocabulary.from_tokenizer(object())
    with pytest.raises(ValueError, match="eos id 9"):
        Vocabulary([b"a"], eos_ids=(9,))
