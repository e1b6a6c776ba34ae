"""The option parser of `kiss` without a device: command lines that break one or two rules (an option without the one it goes
with, a value out of range, a missing value, an unknown option), and a few that break none and stop at the missing input file.
Exit status, stdout and stderr are compared with tests/golden/cli_parse_recording.json, which `record()` below wrote from the
binary of commit a0b0b58, whose parser was an if-chain: which of two broken rules is reported is behaviour."""
import itertools
import json
import os
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KISS = os.path.join(ROOT, "kiss_amd", "kiss")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_parse_recording.json")
OPTIONS = [["--seeds", "r"], ["--min-seed-len", "3"], ["--both-strands"], ["--chain"], ["--max-gap", "3"], ["--align"], ["--match", "3"],
           ["--align-band", "2"], ["--sam"], ["--overlap", "300"], ["--max-hits", "1"], ["--mates", "m"], ["--ins-min", "2000"],
           ["--pair-pen-max", "3"], ["--rescue"], ["--rescue-width", "0"], ["--rescue-anchors", "2"], ["-q", "ACGT"], ["-g"],
           ["--mismatches", "1"], ["--match", "0"], ["--gap-cost", "70000"], ["--min-seed-len", "0"]]
OTHERS = [[], ["-h"], ["-v"], ["--bogus"], ["--seeds"], ["-k"], ["--devices", "1,,2"], ["--devices", "0,1", "--gpus", "3"], ["-t", "4", "-k", "-1"],
          ["--gpus", "0"], ["--sa-intv", "33"], ["--lookup-len", "15"], ["--mismatches", "4"], ["-n"], ["-"]]


def command_lines():
    """every option alone, every two of them, the others; each with a command and a file that does not exist, and with neither"""
    sets = [o for o in OPTIONS] + [a + b for a, b in itertools.combinations(OPTIONS, 2)] + OTHERS
    return [["fmindex_query"] + c + ["missing/x.fa"] for c in sets] + [c for c in sets] + [["suffix_sort"] + c for c in OTHERS]


def run(kiss, args, usage=None):
    """-> [status, stdout, stderr]; the text of `usage`, where stderr has it, as one word"""
    r = subprocess.run([kiss] + args, capture_output=True, text=True, cwd=ROOT)
    return [r.returncode, r.stdout, r.stderr.replace(usage, "<usage>") if usage else r.stderr]


def record(kiss):
    usage = run(kiss, ["-h"])[2]
    return {"-h": usage, "answers": {" ".join(args): run(kiss, args, usage) for args in command_lines()}}


def test_the_parser_answers_as_it_did():
    with open(GOLDEN) as g:
        usage, recorded = (lambda r: (r["-h"], r["answers"]))(json.load(g))
    lines = command_lines()
    assert sorted(recorded) == sorted(" ".join(a) for a in lines) and len(recorded) > 500
    assert run(KISS, ["-h"]) == [1, "", usage] and usage.count("\n") > 70
    wrong = [a for a in lines if run(KISS, a, usage) != recorded[" ".join(a)]]
    assert not wrong, wrong[:5]
