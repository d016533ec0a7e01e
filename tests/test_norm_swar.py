"""CPU check of the word-wide ASCII helpers of the normalise pre-pass (wordpiece_amd/csrc/utf8_swar.h: norm_ascii_lower,
norm_ascii_dropped16, norm_ascii16) against the per-byte rules of norm_cp: compiled with g++, no GPU
(tests/cpp/test_norm_swar.cpp says what is enumerated).

That it bites: three one-token changes of the header, each on a scratch copy, each compiled with the same test and run once.
  - norm_ascii_lower with 0x25252525 -> 0x24242424 ('[' taken for a capital): FAILED, 8,290,815 of the 268,435,456 words
    differ, the first 0000005b -> 0000007b;
  - norm_ascii_dropped16 with 0x60606060 -> 0x61616161 (U+001F kept): FAILED on the single-value chunks, the first
    `1f 61 61 ...`: dropped 0000, expected 0001;
  - norm_ascii_dropped16 without is(0x7fu) (U+007F kept): FAILED on the single-value chunks, the first `7f 61 61 ...`:
    dropped 0000, expected 0001.
The unchanged header passes: 268,435,456 words lowered, 4,032,768 chunks, under two seconds."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_swar_ascii_helpers_equal_the_per_byte_rules(tmp_path):
    exe = str(tmp_path / "test_norm_swar")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_norm_swar.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
