"""The ABI shim's JSON reader and the parameter readers behind it (csrc/shim_json.hpp, shim_json.cpp) in a program of their own
(tests/shim_json_check.cpp) under the host sanitizers, over untrusted bytes: every truncation and the seeded mutations of two real
job bodies, the bodies and numbers tests/test_abi_shim.py sends through the library, and hand-written edge cases.  Every answer
is compared with Python's json made strict; the reader's three limits of its own -- nesting at most 64 deep, a number of at most
64 characters, a finite double -- are the only cases where it may refuse what Python takes, in the words it has today."""
import json
import os
import random
import struct
import subprocess

import pytest

from tests.shim_jobs import GRAMMAR_NUMBERS, INVALID_BODIES, MUTATED_JOBS    # (tests/test_abi_shim.py sends the same through the library)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

REFUSED = object()                                               # python_reads: Python's json does not take the case
LIMIT_TEXTS = ("nesting too deep", "number too long", "number out of range")
FILTERS = {"robidoux_fast": 1, "robidoux": 2, "robidoux_sharp": 3, "ginseng": 4, "ginseng_sharp": 5, "lanczos": 6, "lanczos_sharp": 7, "lanczos_2": 8,
           "lanczos_2_sharp": 9, "cubic": 11, "cubic_sharp": 12, "catmull_rom": 13, "mitchell": 14, "cubic_b_spline": 15, "hermite": 16, "jinc": 17,
           "triangle": 22, "linear": 23, "box": 24, "fastest": 27, "n_cubic": 29, "n_cubic_sharp": 30}     # imageflow_types/src/lib.rs:144-205


def documents():
    """the 'J' cases: (name, bytes)"""
    cases = []
    rnd = random.Random(11)
    for k, job in enumerate(MUTATED_JOBS):
        body = json.dumps(job).encode()
        cases += [("job %d cut at %d" % (k, n), body[:n]) for n in range(len(body) + 1)]
        for i in range(600):                                     # test_json_reader_survives_mutated_jobs' mutations, draw for draw
            m = bytearray(body)
            for _ in range(rnd.randint(1, 5)):
                m[rnd.randrange(len(m))] = rnd.choice(b'{}[]",:0123456789truefalsn\\ \x00\xff' + bytes([rnd.randrange(256)]))
            if rnd.random() < 0.2:
                m = m[:rnd.randrange(1, len(m))]
            rnd.choice(["v1/execute", "v1/build"])               # (the endpoint that test sends it to: the same stream of draws)
            cases.append(("job %d mutation %d" % (k, i), bytes(m)))
    cases += [("invalid body %d" % i, b) for i, b in enumerate(INVALID_BODIES)]
    for n in GRAMMAR_NUMBERS:
        cases.append(("number %r" % n, n))
        cases.append(("number %r in a job" % n, b'{"framewise":{"steps":[{"create_canvas":{"w":' + n + b',"h":8,"format":"bgra_32","color":"transparent"}}]}}'))
    edge = {
        "escapes": rb'"\" \\ \/ \b \f \n \r \t"', "escape u0000": rb'"a\u0000b"', "escape u00e9": rb'"\u00e9"', "escape u00E9": rb'"\u00E9"',
        "escape u20ac": rb'"\u20ac"', "escape u007f u0080 u07ff u0800 uffff": rb'"\u007f\u0080\u07ff\u0800\uffff"', "escaped key": rb'{"A\n": 1}',
        "short u escape": rb'"\u12"', "u escape at the end": rb'"\u', "bad hex digit": rb'"\u12g4"', "bad escape": rb'"\x41"', "escape at the end": b'"\\',
        "control byte": b'"a\x01b"', "newline in a string": b'"a\nb"', "tab in a string": b'"a\tb"', "del in a string": b'"a\x7fb"',
        "unterminated string": b'"abc', "nesting 64 arrays": b"[" * 64 + b"]" * 64, "nesting 65 arrays": b"[" * 65 + b"]" * 65,
        "nesting 63 arrays and a number": b"[" * 63 + b"1" + b"]" * 63, "nesting 64 arrays and a number": b"[" * 64 + b"1" + b"]" * 64,
        "nesting 64 objects": b'{"a":' * 63 + b"{}" + b"}" * 63, "nesting 65 objects": b'{"a":' * 64 + b"{}" + b"}" * 64,
        "number of 64 characters": b"1" + b"0" * 63, "number of 65 characters": b"1" + b"0" * 64, "fraction of 64 characters": b"0." + b"3" * 62,
        "fraction of 65 characters": b"0." + b"3" * 63, "negative of 65 characters": b"-" + b"1" * 64, "1e308": b"1e308", "1e309": b"1e309",
        "-1e309": b"-1e309", "1e-400": b"1e-400", "largest double": b"1.7976931348623157e308", "just above it": b"1.7976931348623159e308",
        "-0": b"-0", "-0.0": b"-0.0", "0": b"0", "exponent forms": b"[1E5, 1e+5, 1e-5, 0e0, 0.5e1, 123456789012345678901234567890]",
        "seventeen digits": b"[0.1, 0.30000000000000004, 9007199254740993, 5e-324, 2.2250738585072014e-308]",
        "empty object": b"{}", "empty array": b"[]", "empty containers nested": b'{"a": [], "b": {}, "c": [{}, []]}', "empty key": b'{"": 0}',
        "duplicate keys": b'{"a": 1, "a": 2, "b": 3, "a": {"a": 4}}', "whitespace of all four kinds": b' \t\r\n{ \t\r\n"a" \t\r\n: \t\r\n[ \t\r\n1 \t\r\n, \t\r\n2 \t\r\n] \t\r\n} \t\r\n',
        "form feed is no whitespace": b"\x0c1", "vertical tab is no whitespace": b"[1,\x0b2]", "no-break space is no whitespace": b"\xc2\xa01",
        "utf-8 passed through raw": "{\"grüße\": \"€ 中文 \U0001f600\"}".encode(), "byte order mark": b"\xef\xbb\xbf{}",
        "literals": b"[true, false, null]", "bare true": b"true", "bare null": b"null", "bare string": b'"x"', "cut literal": b"tru", "wrong literal": b"nul1",
        "capital literal": b"True", "NaN": b"NaN", "-Infinity": b"-Infinity", "trailing comma in an array": b"[1,]", "trailing comma in an object": b'{"a":1,}',
        "missing colon": b'{"a" 1}', "missing comma": b"[1 2]", "key without quotes": b"{a: 1}", "single quotes": b"{'a': 1}", "comment": b"[1 /* no */]",
        "two documents": b"{} {}", "only whitespace": b" \n", "a nul byte": b"\x00", "nul behind a document": b"{}\x00", "minus then letter": b"-a",
        "dot exponent": b"1.e5", "exponent without digits": b"1e", "exponent sign without digits": b"1e+", "double minus": b"--1", "leading zeros": b"-012",
    }
    cases += sorted(edge.items())
    return cases


def parameters():
    """the 'P' cases: (name, call, expected line) -- expectations read off csrc/shim_json.cpp and the reference lines it cites"""
    def value(v):
        return b"V %d" % v
    node, js = b"E 2 InvalidNodeParams: node: bad colour '%s'", b"E 3 InvalidJson: "
    hexc = lambda s: {"srgb": {"hex": s}}                                                         # noqa: E731
    cases = [
        ("colour transparent", {"fn": "parse_color", "arg": "transparent"}, value(0)), ("colour black", {"fn": "parse_color", "arg": "black"}, value(0xFF000000)),
        ("colour null", {"fn": "parse_color", "arg": None}, value(0)), ("colour absent", {"fn": "parse_color"}, value(0)),
        ("colour #abc", {"fn": "parse_color", "arg": hexc("#abc")}, value(0xFFAABBCC)), ("colour abcd", {"fn": "parse_color", "arg": hexc("abcd")}, value(0xDDAABBCC)),
        ("colour 112233", {"fn": "parse_color", "arg": hexc("112233")}, value(0xFF112233)), ("colour 11223344", {"fn": "parse_color", "arg": hexc("11223344")}, value(0x44112233)),
        ("colour 12345", {"fn": "parse_color", "arg": hexc("12345")}, node % b"12345"), ("colour GG0000", {"fn": "parse_color", "arg": hexc("GG0000")}, node % b"GG0000"),
        ("colour of nine digits", {"fn": "parse_color", "arg": hexc("112233445")}, node % b"112233445"), ("colour empty", {"fn": "parse_color", "arg": hexc("")}, node % b""),
        ("colour red", {"fn": "parse_color", "arg": "red"}, js + b"node: unknown colour 'red'"),
        ("colour a number", {"fn": "parse_color", "arg": 5}, js + b'node: colour must be "transparent", "black" or {"srgb":{"hex":..}}'),
        ("colour hex a number", {"fn": "parse_color", "arg": hexc(5)}, js + b'node: colour must be "transparent", "black" or {"srgb":{"hex":..}}'),
        ("keyword transparent", {"fn": "keyword_transparent", "arg": "transparent"}, value(1)), ("keyword null", {"fn": "keyword_transparent", "arg": None}, value(1)),
        ("keyword absent", {"fn": "keyword_transparent"}, value(1)), ("keyword black", {"fn": "keyword_transparent", "arg": "black"}, value(0)),
        ("keyword srgb of alpha 0", {"fn": "keyword_transparent", "arg": hexc("00000000")}, value(0)),
        ("int 7", {"fn": "want_int", "arg": 7}, value(7)), ("int -7", {"fn": "want_int", "arg": -7}, value(-7)), ("int 2^53", {"fn": "want_int", "arg": 2 ** 53}, value(2 ** 53)),
        ("int -2^53", {"fn": "want_int", "arg": -2 ** 53}, value(-2 ** 53)), ("int 1.5", {"fn": "want_int", "arg": 1.5}, js + b"node.arg must be an integer"),
        ("int 2^53+2", {"fn": "want_int", "arg": 2 ** 53 + 2}, js + b"node.arg must be an integer"), ("int a string", {"fn": "want_int", "arg": "7"}, js + b"node.arg must be an integer"),
        ("int absent", {"fn": "want_int"}, js + b"node.arg must be an integer"), ("u32 0", {"fn": "want_u32", "arg": 0}, value(0)),
        ("u32 2^31-1", {"fn": "want_u32", "arg": 2 ** 31 - 1}, value(2 ** 31 - 1)), ("u32 -1", {"fn": "want_u32", "arg": -1}, js + b"node.arg out of range"),
        ("u32 2^31", {"fn": "want_u32", "arg": 2 ** 31}, js + b"node.arg out of range"), ("u32 1.5", {"fn": "want_u32", "arg": 1.5}, js + b"node.arg must be an integer"),
        ("filter absent", {"fn": "parse_filter"}, value(-1)), ("filter null", {"fn": "parse_filter", "arg": None}, value(-1)),
        ("filter unknown", {"fn": "parse_filter", "arg": "bicubic"}, js + b"unknown filter"), ("filter a number", {"fn": "parse_filter", "arg": 2}, js + b"unknown filter"),
        ("filter in capitals", {"fn": "parse_filter", "arg": "Robidoux"}, js + b"unknown filter"),
        ("coder absent", {"fn": "encode_coder"}, value(0)), ("coder gif", {"fn": "encode_coder", "arg": "gif"}, value(0)),
        ("coder webplossless", {"fn": "encode_coder", "arg": "webplossless"}, None), ("coder libjpeg_turbo", {"fn": "encode_coder", "arg": {"libjpeg_turbo": {}}}, None),
        ("coder libpng", {"fn": "encode_coder", "arg": {"libpng": {}}}, None), ("coder pngquant", {"fn": "encode_coder", "arg": {"pngquant": {}}}, None),
        ("coder mozjpeg", {"fn": "encode_coder", "arg": {"mozjpeg": {}}}, None),
    ]
    cases += [("filter " + name, {"fn": "parse_filter", "arg": name}, value(v)) for name, v in FILTERS.items()]
    assert len(FILTERS) == 22
    return cases


def python_reads(case):
    """-> (value, or REFUSED when Python's json refuses; the reader's limits the document is beyond).  Bytes that are no UTF-8 stay
    what they are (surrogateescape: the reader hands a string's bytes on as they come), every number is read as a double."""
    beyond = set()

    def number(token):
        if len(token) > 64:
            beyond.add("number too long")
        try:
            v = float(token)
        except OverflowError:
            v = float("inf")
        if v in (float("inf"), float("-inf")):
            beyond.add("number out of range")
        return v

    def constant(token):
        raise ValueError("no JSON: " + token)

    def depth(v):                                                # every value counts, a scalar too
        return 1 + max([depth(x) for x in (v.values() if isinstance(v, dict) else v)] or [0]) if isinstance(v, (dict, list)) else 1

    try:
        v = json.loads(case.decode("utf-8", "surrogateescape"), parse_float=number, parse_int=number, parse_constant=constant)
    except ValueError:
        return REFUSED, beyond
    if depth(v) > 64:
        beyond.add("nesting too deep")
    return v, beyond


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("shim_json")
    exe, blob = str(tmp / "shim_json_check"), str(tmp / "cases.bin")
    csrc = os.path.join(ROOT, "imageflow_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", csrc, "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "shim_json_check.cpp"), os.path.join(csrc, "shim_json.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)                  # (no skip where no sanitizer runtime links: this is the reader's only run under one)
    assert built.returncode == 0, built.stderr[-3000:]
    docs, params = documents(), parameters()
    with open(blob, "wb") as f:
        for _, data in docs:
            f.write(b"J" + struct.pack("<I", len(data)) + data)
        for _, call, _ in params:
            data = json.dumps(call).encode()
            f.write(b"P" + struct.pack("<I", len(data)) + data)
    r = subprocess.run([exe, blob], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:].decode("utf-8", "replace")        # (-fno-sanitize-recover=all: a finding ends the program)
    assert r.stderr == b""
    lines = r.stdout.split(b"\n")
    assert lines[-1] == b"" and len(lines) - 1 == len(docs) + len(params)        # (no answer holds a line feed: to_json escapes them, the messages here have none)
    return docs, lines[:len(docs)], params, lines[len(docs):-1]


def test_the_corpus_is_what_the_issue_lists():
    docs = documents()
    names = [n for n, _ in docs]
    assert len(set(names)) == len(names)
    for k, job in enumerate(MUTATED_JOBS):                       # every truncation, 600 mutations
        assert sum(n.startswith("job %d cut at " % k) for n in names) == len(json.dumps(job)) + 1
        assert sum(n.startswith("job %d mutation " % k) for n in names) == 600
    assert not any(rb"\ud" in d.lower() for _, d in docs)       # surrogate escapes: Python and the reader differ by design, none here


def test_the_reader_takes_what_json_takes_and_refuses_what_it_refuses(answers):
    docs, lines, _, _ = answers
    taken = refused = at_limit = 0
    for (name, case), line in zip(docs, lines):
        want, beyond = python_reads(case)
        assert not line.startswith(b"U "), (name, line[:200])                      # to_json is stable: its text reads back to the same text
        if want is REFUSED:
            assert line.startswith(b"E 3 InvalidJson: "), (name, case[:200], line[:200])
            refused += 1
        elif beyond:                                                               # the reader's own limits, in its own words
            assert line.startswith(b"E 3 InvalidJson: ") and any(line.startswith(b"E 3 InvalidJson: " + t.encode() + b" at byte ") for t in beyond), (name, beyond, line[:200])
            at_limit += 1
        else:
            assert line.startswith(b"S "), (name, case[:200], line[:200])
            got, _ = python_reads(line[2:])
            assert got == want, (name, case[:200], line[:200])
            taken += 1
    print("taken", taken, "refused", refused, "at a limit", at_limit)
    assert taken > 100 and refused > 2000 and at_limit >= 10, (taken, refused, at_limit)


@pytest.mark.parametrize("name, text", [("nesting 64 arrays", None), ("nesting 65 arrays", "nesting too deep"), ("nesting 63 arrays and a number", None),
                                        ("nesting 64 arrays and a number", "nesting too deep"), ("nesting 64 objects", None), ("nesting 65 objects", "nesting too deep"),
                                        ("invalid body 5", "nesting too deep"), ("number of 64 characters", None), ("number of 65 characters", "number too long"),
                                        ("fraction of 64 characters", None), ("fraction of 65 characters", "number too long"), ("negative of 65 characters", "number too long"),
                                        ("1e308", None), ("1e309", "number out of range"), ("-1e309", "number out of range"), ("largest double", None),
                                        ("just above it", "number out of range"), ("number b'1e999'", "number out of range"), ("1e-400", None)])
def test_the_three_limits_are_refused_in_todays_words(answers, name, text):
    docs, lines, _, _ = answers
    line = lines[[n for n, _ in docs].index(name)]
    if text is None:
        assert line.startswith(b"S "), line[:200]
    else:
        assert text in LIMIT_TEXTS and line.startswith(b"E 3 InvalidJson: " + text.encode() + b" at byte "), line[:200]


def test_answers_that_are_pinned_byte_for_byte(answers):
    docs, lines, _, _ = answers
    got = dict(zip((n for n, _ in docs), lines))
    assert got["-0"] == b"S -0" and got["0"] == b"S 0" and got["empty object"] == b"S {}" and got["empty array"] == b"S []"
    assert got["escape u0000"] == rb'S "a\u0000b"' and got["escape u00e9"] == 'S "é"'.encode() and got["escape u20ac"] == 'S "€"'.encode()
    assert got["escapes"] == rb'S "\" \\ / \u0008 \u000c \u000a \u000d \u0009"'
    assert got["duplicate keys"] == b'S {"a":1,"a":2,"b":3,"a":{"a":4}}'            # every pair is kept, in order; JVal::get answers with the first
    assert got["whitespace of all four kinds"] == b'S {"a":[1,2]}'
    assert got["utf-8 passed through raw"] == 'S {"grüße":"€ 中文 \U0001f600"}'.encode()
    assert got["short u escape"].startswith(b"E 3 InvalidJson: short \\u escape at byte ") and got["bad hex digit"].startswith(b"E 3 InvalidJson: bad hex digit at byte ")
    assert got["control byte"].startswith(b"E 3 InvalidJson: control character in string at byte ")
    assert got["job 0 cut at %d" % len(json.dumps(MUTATED_JOBS[0]))].startswith(b'S {"io":[{"io_id":0,')


def test_the_parameter_readers_answer_as_their_code_says(answers):
    _, _, params, lines = answers
    for (name, call, want), line in zip(params, lines):
        if want is not None:
            assert line == want, (name, line)
    got = {name: line for (name, _, _), line in zip(params, lines)}
    coders = [got["coder " + k] for k in ("absent", "libjpeg_turbo", "libpng", "pngquant", "mozjpeg", "webplossless")]
    assert all(c.startswith(b"V ") for c in coders) and len(set(coders)) == 6       # IFHIP_ENCODE_CODER_*: six coders, six numbers
