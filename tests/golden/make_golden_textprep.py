#!/usr/bin/env python3
"""Generate tests/golden/textprep.json by running the REFERENCE's Processors.word_cleaner / word_cleaner_lower (sam/datasets/processors.py:746-755) on CPU.

Runs ONLY in the build container (the reference never travels to the GPU box); the processor module is imported with the shims of
make_golden_answers.py.  Contents:
  whitespace   the code points c with chr(c).isspace(), enumerated over all of Unicode by the interpreter that ran the reference
  cases        [{"s": the raw string, "word_cleaner": ..., "word_cleaner_lower": ...}] for a few hundred strings: realistic OCR tokens and answers, the
               possessive cases, strings that clean to nothing, every whitespace code point at both ends and in the middle, 2-, 3- and 4-byte code
               points, and the strings on which str.lower() is not an ASCII matter (I with dot above, capital sharp s, the Kelvin sign, final sigma)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_textprep.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden.make_golden_answers import import_processor  # noqa: E402

REALISTIC = [
    "STOP", "Coca-Cola", "coca cola", "EXIT", "Joe's", "JOE'S", "McDonald's", "what?", "1,000", "12,345,678", "Hello, World", "U.S.A.", "No.", "5th Ave", "OPEN 24 HOURS",
    "www.example.com", "info@example.org", "$3.99", "50%", "#1", "(stop)", "[sic]", "don't", "DON'T", "it's", "IT'S", "its", "Levi's 501", "men's room", "the cat's hat",
    "Is this a dog?", "yes", "no", "unanswerable", "blue and white", "10:30", "3/4", "a-b-c", "one,two,three", "who?what?where?", "???", "St. John's", "rock 'n' roll",
    "'tis", "o'clock", "O'CLOCK", "kids' menu", "boss's", "BOSS'S", "Paris, France", "  padded  ", "\tTabbed\t", "line\nbreak", "trailing,", ",leading", "mid,dle",
    "A", "a", "Z", "z", "AZ az", "0123456789", "MiXeD cAsE", "ALL CAPS TOKEN", "what's the name of the store?", "How many's there?", "s", "S", "'", "?", ",",
    "toys'r'us", "samsung", "NOKIA", "LG", "h&m", "7-eleven", "p.m.", "A.M.", "25 mph", "EST. 1984", "no parking", "ONE WAY", "what time is it?", "12:00, noon",
]
POSSESSIVE = [
    "'s", "'S", "'?s", "',s", "''s", "'ss", "'", "s'", "x'", "x's", "x'S", "x'?s", "x',s", "x''s", "x'ss", "x's's", "X'S'S", "'s's", "'s 's", " 's", "  's  ", "'s ", "a 's",
    "a  's", "'?,?s", "'?", "'?x", "'sx", "''", "'''s", "s's", "s'ss's", "'s?", "?'s", ",'s", "'s,", "'s'", "it's joe's", "'S ", " 'S", "a'š", "a'ſ", "é's", "É'S",
]
TO_EMPTY = ["", " ", "  ", ",", "?", ",?", "?,", " , ? ", "\t", "\n", " \t\n\r\x0b\x0c ", "　", ",,,,", "????", " ?"]
MULTIBYTE = [
    "café", "CAFÉ", "naïve", "über", "ÜBER", "straße", "ñ", "Ñ", "αβγ", "ΑΒΓ", "привет",
    "ПРИВЕТ", "中文", "日本語", "한글", "ไทย", "€5", "™", "—dash—", "“quoted”",
    "’s", "x’s", "\U0001f600", "\U0001f600's", "a\U0001f600b", "\U00010400", "\U00010428", "\U0001d11e clef", "\U0010ffff", "߿", "ࠀ", "￿", "\U00010000",
    "\x7f", "\x80", "\x00", "a\x00b", "é,é?é's", "中's", "中, 文?",
]
LOWERING = [
    "İ", "İstanbul", "İS", "ẞ", "STRAẞE", "K", "Kelvin", "5 K", "Σ", "ΟΔΟΣ", "ΟΔΟΣ Α",
    "ΣΣ", "aΣ", "AΣ", "Σ's", "İ's", "K'S", "K, K?", "ǅ", "Ǆ", "ﬁ", "Ⅰ", "Ⓐ", "µ", "ẞ'S ",
]


def main():
    P, _ = import_processor()
    wc, wcl = P.Processors.word_cleaner, P.Processors.word_cleaner_lower
    ws = [c for c in range(0x110000) if chr(c).isspace()]
    strings = REALISTIC + POSSESSIVE + TO_EMPTY + MULTIBYTE + LOWERING
    for c in ws:
        w = chr(c)
        strings += [w + "Ab" + w + "Cd" + w, w + w + "x's" + w + w, "q" + w + "'s", w]
    strings += [" ".join(REALISTIC[i:i + 3]) for i in range(0, len(REALISTIC), 3)]
    seen, cases = set(), []
    for s in strings:
        if s in seen:
            continue
        seen.add(s)
        s.encode("utf-8")                                        # (no lone surrogates: every case can be shipped)
        cases.append({"s": s, "word_cleaner": wc(s), "word_cleaner_lower": wcl(s)})
    with open(os.path.join(HERE, "textprep.json"), "w") as f:
        json.dump({"whitespace": ws, "cases": cases}, f, indent=0, ensure_ascii=True)
        f.write("\n")
    print("textprep.json: %d cases, %d whitespace code points, %.1f KB" % (len(cases), len(ws), os.path.getsize(os.path.join(HERE, "textprep.json")) / 1024))


if __name__ == "__main__":
    main()
