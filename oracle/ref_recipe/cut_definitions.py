#!/usr/bin/env python3
"""ORACLE -- TEST INFRASTRUCTURE ONLY.
Cuts whole definitions out of a C++ source file at build time, by the text their first line begins with and by brace matching
(never by line number), and writes them, unmodified and in the order asked for, inside one namespace block.

    cut_definitions.py OUT NAMESPACE SOURCE PREFIX [PREFIX ...] [-- SOURCE PREFIX ...]

A PREFIX that ends in '=' names a statement (cut up to its ';'); every other PREFIX names a function definition (cut from its
first line to the brace that closes its body).  Comments, string and character literals are skipped while braces are counted.
A PREFIX that matches no line, or more than one, is an error: the recipe fails rather than compile something else.

oracle/Makefile (ref_stereo) uses this for the functions of the reference's src/Frame.cc that the stereo pin drives; the output
lands in oracle/_ref/, which is never committed.
"""
import sys


def _strip(line):
    return " ".join(line.split())


def _end_of_body(text, start):
    """Index just past the brace that closes the first '{' at or after start."""
    i, depth, n = start, 0, len(text)
    while i < n:
        c = text[i]
        two = text[i:i + 2]
        if two == "//":
            i = text.index("\n", i) if "\n" in text[i:] else n
            continue
        if two == "/*":
            i = text.index("*/", i + 2) + 2
            continue
        if c in "\"'":
            j = i + 1
            while text[j] != c:
                j += 2 if text[j] == "\\" else 1
            i = j + 1
            continue
        if c == "{":
            depth += 1
        elif c == "}":
            depth -= 1
            if depth == 0:
                return i + 1
        elif c == ";" and depth == 0:
            raise SystemExit("cut_definitions: a declaration, not a definition, at offset %d" % start)
        i += 1
    raise SystemExit("cut_definitions: unbalanced braces after offset %d" % start)


def cut(path, prefixes):
    text = open(path, encoding="utf-8", errors="surrogateescape").read()
    offsets, o = [], 0
    for line in text.splitlines(keepends=True):
        offsets.append((o, _strip(line)))
        o += len(line)
    out = []
    for p in prefixes:
        want = _strip(p)
        hits = [off for off, s in offsets if s.startswith(want)]
        if len(hits) != 1:
            raise SystemExit("cut_definitions: %r matches %d lines of %s" % (p, len(hits), path))
        start = hits[0]
        end = text.index(";", start) + 1 if want.endswith("=") else _end_of_body(text, start)
        out.append(text[start:end])
    return out


def main(argv):
    if len(argv) < 5:
        raise SystemExit(__doc__)
    out_path, namespace, rest = argv[1], argv[2], argv[3:]
    groups, cur = [], []
    for a in rest:
        if a == "--":
            groups.append(cur); cur = []
        else:
            cur.append(a)
    groups.append(cur)
    pieces = []
    for g in groups:
        pieces += cut(g[0], g[1:])
    with open(out_path, "w", encoding="utf-8", errors="surrogateescape") as f:
        f.write("namespace %s {\n\n" % namespace)
        f.write("\n\n".join(pieces))
        f.write("\n\n}\n")


if __name__ == "__main__":
    main(sys.argv)
