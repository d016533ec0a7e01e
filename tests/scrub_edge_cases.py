"""Constructed and seeded random batches for the scrub (csrc/scrub.h, scrub_path.h) past its first tile and its first grid, with
what every case claims.  Shared by the model-only tests and the GPU tests of test_gpu_scrub_edges.py.  Importing this module
loads no library; the expected results come from scrub_model alone.

CASES[name] = (rows, how, claim): the rows of a batch, the keywords of the scrub calls, and claim(exp, off), which asserts on
the model's answer that the case is the case its name says (off: the row offsets).

group (issue bullet)                                  cases
1  n rows, n at the wave, workgroup and scan-tile     rows <n> plain, rows <n> rules   (n = 1 63 64 255 256 257 2047 2048 2049)
   edges; rules that fail rows in a partial wave
2  > kBlock row starts in one span, over a tile       tiny rows over a tile start
   start; empty rows first; > kBlock empty rows last  empty rows first, empty rows last
   a row start at T - 1, T, 2 T with a match that     boundary <T-1|T|2T> <email|ipv4> <ends|starts|cut>
   ends in front of it, starts on it, is cut by it
3  1 5 6 T-1 T T+1 2T 2T+1 bytes that end in '@',     size <n> <at|email|ipv4> <one row|two rows>
   in a@b.cc, in 1.2.3.4; one row, two rows cut at T
4  addresses inside e-mails: the domain part (short,  inside e-mails, inside e-mails, ipv4 only
   as late as a domain of 255 allows with the '@' in
   the tile in front, a domain of 256), local runs of
   64 and 65 over a tile end, an e-mail that ends in
   front, an '@' in the row in front
5  nm + 1 at the scan tile; a tile up against         list <nm>   (nm = 2047 2048 2049)
   kScTileMatches at 6-byte spacing; both kinds       dense tile, dense tile of both kinds
6  seeded random rows of near-misses and fragments    random <seed> replaced, random <seed> private   (seed = 0 1 2)"""
import os
import random
import re

import scrub_model as M

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wordpiece_amd", "csrc")
# the numbers the cases are built from, as the sources write them (geometry() holds the sources to them)
SOURCE = {"common.h": {"kWave": "64", "kBlock": "256"}, "quality.h": {"kQualItems": "8", "kQualTile": "kBlock * kQualItems"},
          "scrub.h": {"kScFront": "328", "kScBehind": "328", "kScTileMatches": "kQualTile / 6 + 2"},
          "primitives.h": {"kScanItems": "8", "kScanTile": "kBlock * kScanItems"}}
WAVE, BLOCK, ITEMS = 64, 256, 8
T = BLOCK * ITEMS              # kQualTile: the bytes of a tile of the three tiled kernels
FRONT = BEHIND = 328           # kScFront, kScBehind: the halo of the find kernel
TILE_MATCHES = T // 6 + 2      # kScTileMatches: the matches a tile of the write kernel stages
SCAN_TILE = BLOCK * 8          # kScanTile: the entries a workgroup of device_exclusive_scan takes


def geometry():
    """-> {name: the text of its value} of every constant of SOURCE as the headers define it"""
    out = {}
    for header, names in SOURCE.items():
        with open(os.path.join(CSRC, header)) as f:
            src = f.read()
        for name in names:
            m = re.search(r"^constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, src, re.M)
            assert m, (header, name)
            out[name] = m.group(1).strip()
    return out


def offsets(rows):
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r))
    return off


def pad(n):
    """n bytes of plain text without a match that end in a blank"""
    return (b"some text, no match. " * (n // 21 + 1))[:n - 1] + b" " if n > 0 else b""


def signals_of(exp, row):
    return tuple(exp["signals"][M.S[k]][row] for k in ("emails", "ips", "ips_left"))


CASES = {}
LISTS = dict(email=[b"", b"<e>", b"E" * 64, b"mail"], ip=[b"", b"<an address, a longer one>", b"i"])

# ---- 1. row counts ---------------------------------------------------------------------------------------------------------------
ROW_COUNTS = (1, WAVE - 1, WAVE, BLOCK - 1, BLOCK, BLOCK + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1)


def short_row(i):
    """every third row holds an e-mail or an address (every twelfth a private one); of the others some are empty, some '@'"""
    if i % 3 == 0:
        return b"%c@b.cc" % (97 + i % 26) if i % 6 == 0 else (b"10.0.0.1" if i % 12 == 9 else b"8.8.8.%d" % (i % 250))
    return (b"", b"@", b"xy", b"1.")[(i // 3 + i) % 4]


for _n in ROW_COUNTS:
    _rows = [short_row(i) for i in range(_n)]

    def _claim(exp, off, n=_n):
        st = exp["stats"]
        assert st["n_rows"] == n and st["n_matches"] == [(n + 5) // 6, (n + 2) // 6, 0] and st["n_kept"] == n, st

    def _claim_rules(exp, off, n=_n):
        st = exp["stats"]  # max_emails 0 fails the e-mail rows, max_ips 0 the address rows, the private ones among them
        assert st["rule_failed"] == [(n + 5) // 6, (n + 2) // 6] and st["n_kept"] == n - sum(st["rule_failed"]), st
        assert st["n_matches"][2] == (n + 2) // 12

    CASES["rows %d plain" % _n] = (_rows, LISTS, _claim)
    CASES["rows %d rules" % _n] = (_rows, dict(rules={"max_emails": 0, "max_ips": 0}, keep_private=True), _claim_rules)

# ---- 2. many row starts in one span; row starts on tile starts ------------------------------------------------------------------
_tiny = [x for k in range(300) for x in (b"", b"a@b.cc 1.2.3.4 "[k % 15:k % 15 + 1])]  # 600 rows, 300 bytes: a match cut into rows of one byte


def _claim_tiny(exp, off):
    assert sum(T - FRONT <= o < T + BEHIND for o in off[:-1]) > 2 * BLOCK and off[1] < T < off[601]  # the run lies across the tile start
    assert all(signals_of(exp, r) == (0, 0, 0) for r in range(1, 601)) and exp["stats"]["n_matches"][0] >= 20


CASES["tiny rows over a tile start"] = ([(b"mail a@b.cc or 10.0.0.1 now. " * 80)[:T - 150]] + _tiny + [b" a@b.cc 8.8.8.8 " * 20], LISTS, _claim_tiny)
def expect(what, want):
    """-> a claim: what(exp) is `want`"""
    def claim(exp, off):
        assert what(exp) == want, (what(exp), want)
    return claim


CASES["empty rows first"] = ([b""] * (BLOCK + 44) + [b"a@b.cc", b"1.2.3.4 x", b"", b"x 9.9.9.9"], LISTS,
                             expect(lambda exp: [signals_of(exp, BLOCK + 44 + k) for k in range(4)], [(1, 0, 0), (0, 1, 0), (0, 0, 0), (0, 1, 0)]))
CASES["empty rows last"] = ([b"x a@b.cc", b"8.8.8.8"] + [b""] * (BLOCK + 44), dict(LISTS, rules={"max_ips": 0}),
                            expect(lambda exp: (exp["stats"]["n_matches"], exp["stats"]["n_kept"]), ([1, 1, 0], BLOCK + 45)))
for _bname, _bd in (("T-1", T - 1), ("T", T), ("2T", 2 * T)):
    for _kind, _m in (("email", b"ab@cd.ee"), ("ipv4", b"8.8.8.8")):
        def _claim_at(start, bd=_bd):
            def claim(exp, off):
                assert off[1] == bd and (start is None or start in exp["match_start"])
                assert start is not None or not [s for s in exp["match_start"] if bd - 8 <= s < bd + 8]
            return claim
        CASES["boundary %s %s ends" % (_bname, _kind)] = ([pad(_bd - len(_m)) + _m, b"next row x@y.zz 9.9.9.9"], LISTS, _claim_at(_bd - len(_m)))
        CASES["boundary %s %s starts" % (_bname, _kind)] = ([pad(_bd), _m + b" and a tail"], LISTS, _claim_at(_bd))
        CASES["boundary %s %s cut" % (_bname, _kind)] = ([pad(_bd - 3) + _m[:3], _m[3:] + b" and a tail"], LISTS, _claim_at(None))

# ---- 3. data sizes -------------------------------------------------------------------------------------------------------------
SIZES = (1, 5, 6, T - 1, T, T + 1, 2 * T, 2 * T + 1)
for _n in SIZES:
    for _tname, _tail in (("at", b"@"), ("email", b"a@b.cc"), ("ipv4", b"1.2.3.4")):
        _data = (pad(_n) + _tail)[-_n:]
        for _form, _cut in (("one row", None), ("two rows", min(T, _n))):
            def _claim_size(exp, off, n=_n, tail=_tail, cut=_cut):
                assert off[-1] == n and exp["stats"]["n_bytes"] == n
                whole = n >= len(tail) and tail != b"@" and (cut is None or not n - len(tail) < cut < n)  # the tail is a match, at the very end
                ends = [s + l for s, l in zip(exp["match_start"], exp["match_len"])]
                assert (ends[-1:] == [n]) == whole, (ends[-3:], n)
            CASES["size %d %s %s" % (_n, _tname, _form)] = ([_data] if _cut is None else [_data[:_cut], _data[_cut:]], {}, _claim_size)

# ---- 4. addresses inside e-mails ------------------------------------------------------------------------------------------------
FILL = b"a" * 63 + b"." + b"b" * 63 + b"." + b"c" * 63 + b"."  # 192 bytes of a domain; d's bring it to 242 or 243
LATE = b"-1.2.3.4-b.cc"      # the address as late as the rules allow: no letter may touch it, no label end in '-', and two letters close a domain


def _inside():
    rows, want, at = [], [], {}

    def add(row, signals):
        rows.append(row)
        want.append(signals)

    def over_tile_end(run):  # the run starts ten bytes in front of the next tile end that leaves room for a blank in front of it
        here = sum(map(len, rows))
        edge = (here + 11 + T - 1) // T * T
        at[len(rows)] = edge - 10
        return pad(edge - 10 - here) + run

    add(pad(T - 201) + b"x@" + FILL + b"d" * 50 + LATE, (1, 0, 0))      # a domain of 255; the '@' at T - 200, the address at T + 44
    add(b"x@a-1.2.3.4-b.com", (1, 0, 0))
    add(b"x@" + FILL + b"d" * 51 + LATE, (0, 1, 0))                      # a domain of 256: no e-mail
    add(over_tile_end(b"1.2.3.4-" + b"x" * 56 + b"@b.cc"), (1, 0, 0))    # a local run of 64
    add(over_tile_end(b"1.2.3.4-" + b"x" * 57 + b"@b.cc"), (0, 1, 0))    # of 65: no e-mail
    add(b"a@b.cc.x-1.2.3.4", (1, 1, 0))                                  # the nearest '@' belongs to an e-mail that ends in front
    add(b"x@a-", (0, 0, 0))                                              # the nearest '@' lies in the row in front
    add(b"1.2.3.4-b.com", (0, 1, 0))
    add(b"x@a.cc-", (0, 0, 0))
    add(b"1.2.3.4-b.com x@a.cc-1.2.3.4-b.com", (1, 1, 0))                # (one row, the second address is inside)
    return rows, want, at


INSIDE_ROWS, INSIDE_WANT, INSIDE_AT = _inside()


def _claim_inside(exp, off):
    data = b"".join(INSIDE_ROWS)
    assert data.index(b"@") == T - 200 and data.index(b"1.2.3.4") == T + 44 and len(FILL + b"d" * 50 + LATE) == 255
    for r, p in INSIDE_AT.items():  # the local runs: the address in front of a tile end, the '@' behind it
        assert data[p:p + 7] == b"1.2.3.4" and p % T == T - 10 and data.index(b"@", p) // T == p // T + 1
    assert [signals_of(exp, r) for r in range(len(INSIDE_ROWS))] == INSIDE_WANT
    suppressed = sum(any(a <= s and e <= b for a, b in M.emails(row)) for row in INSIDE_ROWS for s, e, _ in M.ipv4s(row))
    assert suppressed == 4 and exp["stats"]["n_matches"] == [5, 5, 0]


def _claim_inside_ipv4(exp, off):
    assert exp["stats"]["n_matches"] == [0, 9, 0] and [sum(signals_of(exp, r)) for r in range(len(INSIDE_ROWS))] == [1, 1, 1, 1, 1, 1, 0, 1, 0, 2]


CASES["inside e-mails"] = (INSIDE_ROWS, LISTS, _claim_inside)
CASES["inside e-mails, ipv4 only"] = (INSIDE_ROWS, dict(LISTS, kinds=["ipv4"]), _claim_inside_ipv4)

# ---- 5. list scans -------------------------------------------------------------------------------------------------------------
def _item(i):
    return b"%d.%d.%d.%d " % (1 + i % 200, i % 7, i % 11, 1 + i % 250) if i % 3 == 2 else b"%c@%c.cc " % (97 + i % 26, 97 + i // 26 % 26)


for _nm in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
    _items = [_item(i) for i in range(_nm)]
    CASES["list %d" % _nm] = ([b"".join(_items[k:k + 37]) for k in range(0, _nm, 37)], LISTS,
                              expect(lambda exp: (sum(exp["stats"]["n_matches"]), sorted(set(exp["match_repl"]))), (_nm, [0, 1, 2, 3])))


def _claim_dense(exp, off):  # tile 1 meets as many matches as the write kernel has room for
    assert sum(s < 2 * T and s + l > T for s, l in zip(exp["match_start"], exp["match_len"])) == TILE_MATCHES and exp["stats"]["n_matches"][0] == 1100


CASES["dense tile"] = ([b"xyz"] + [b"%c@b.cc" % (97 + i % 26) for i in range(1100)], LISTS, _claim_dense)
CASES["dense tile of both kinds"] = ([b"%c@b.cc" % (97 + i % 26) if i % 2 else b"1.2.3.%d" % (i % 10) for i in range(1200)], dict(LISTS, keep_private=True),
                                     expect(lambda exp: exp["stats"]["n_matches"], [600, 600, 0]))

# ---- 6. seeded random rows -----------------------------------------------------------------------------------------------------
SEEDS = (0, 1, 2)
ALPHABET = (b"a", b"Z", b"1", b"25", b"0", b".", b"@", b"-", b"_", b"%", b" ", b"\n", "é".encode())
DOMAIN = lambda n: FILL + b"d" * (n - 195) + b".ee"  # noqa: E731  (a domain of n bytes, 196 <= n <= 258)
FRAGMENTS = (
    [b"a@b.cc", b"Bob@Example.COM", b"x_y%z@a-b.c0.org", b"1.a@b.cc", b"u+v@w.info"] +                       # e-mails
    [b"a@b.c", b"a@-b.cc", b"a@b-.cc", b"@b.cc", b"a@@b.cc", b"a@b..cc", b"a@b.c1", b"_@b.cc", b"a@.cc"] +     # almost
    [b"8.8.8.8", b"1.2.3.4", b"100.100.100.100", b"25.25.0.1", b"9.9.9.9.", b" 1.1.1.1 ", b" 8.8.4.4 ", b"11.0.0.1", b"128.0.0.0", b" 172.32.0.1",
     b"192.169.0.1 ", b"223.255.255.255", b" 169.255.0.0 "] +                                                  # addresses
    [b"10.0.0.1", b"192.168.1.1", b"127.0.0.1", b"172.16.0.1", b"169.254.1.1", b"0.0.0.0", b"255.255.255.255"] +  # private
    [b"1.2.3.256", b"01.2.3.4", b"1.2.3", b"1.2.3.4.5", b"1..2.3", b"1.2.3.4x", b"x1.2.3.4", b"1.2.3.4_"] +    # almost
    [b"x@a-1.2.3.4-b.com", b"1.2.3.4-x@y.org", b"1.2.3.4@b.cc", b"u@h.1.2.3.4.org"] +                          # an address inside an e-mail
    [b"x" * n + b"@b.cc" for n in (63, 64, 65)] + [b"x@" + b"a" * n + b".com" for n in (62, 63, 64)] +
    [b"u@" + DOMAIN(n) for n in (254, 255, 256, 257)])
RANDOM_HOW = dict(email=[b"", b"E" * 64, b"<mail>", b"e@x.invalid"], ip=[b"I" * 64, b"", b"<an address>"], rules={"max_emails": 2, "max_ips": 2})


def random_rows(seed):
    """a few hundred to 2,000 short rows of ALPHABET and FRAGMENTS, 3 T to 8 T bytes; in front of every tile start a row is
    laid so that an e-mail crosses the tile start, and the row behind it starts less than 64 bytes behind the tile start"""
    rng = random.Random(seed)
    rows, total, target, planted = [], 0, rng.randint(5 * T, 7 * T), 0
    while total < target:
        while total > (planted + 1) * T - 8:
            planted += 1  # (the rows went over the stretch in front of this tile start)
        edge = (planted + 1) * T
        if total >= edge - 64:
            rows += [b" " * (edge - 3 - total) + b"ab@cd.ee ", b"8.8.8.8 " + rng.choice(FRAGMENTS)]  # the second row starts at edge + 6
            planted += 1
        else:
            n = rng.choice((0, 0, 1, 1, 2, 3, 5, 8))
            rows.append(b"".join(rng.choice(FRAGMENTS) if rng.random() < 0.25 else rng.choice(ALPHABET) for _ in range(n)))
        total = sum(map(len, rows))
    return rows


def random_floors(rows):
    """what the model finds in the rows -> the counts the floors of the issue are about"""
    off = offsets(rows)
    n = dict(rows=len(rows), bytes=off[-1], emails=0, replaced=0, private=0, suppressed=0, crossing=0, behind_tile_start=0)
    for r, row in enumerate(rows):
        es = M.emails(row)
        n["suppressed"] += sum(any(a <= s and e <= b for a, b in es) for s, e, _ in M.ipv4s(row))
        for s, e, kind in M.matches(row, M.EMAIL | M.IPV4 | M.KEEP_PRIVATE):
            n[("emails", "replaced", "private")[kind]] += 1
            n["crossing"] += (off[r] + s) // T != (off[r] + e - 1) // T
            n["behind_tile_start"] += off[r] >= T and off[r] % T < 64
    return n


FLOORS = dict(emails=20, replaced=20, private=3, suppressed=3, crossing=1, behind_tile_start=1)
for _seed in SEEDS:
    _rows = random_rows(_seed)
    CASES["random %d replaced" % _seed] = (_rows, RANDOM_HOW, None)
    CASES["random %d private" % _seed] = (_rows, dict(RANDOM_HOW, keep_private=True), None)

# the cheapest cases of every group, for the runs on the checking builds
HARD = ("rows 257 rules", "rows 2049 plain", "tiny rows over a tile start", "empty rows last", "boundary T email cut", "boundary 2T ipv4 ends", "size 2049 email two rows",
        "size 2048 at one row", "inside e-mails", "list 2048", "dense tile", "random 0 private")
