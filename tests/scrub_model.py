"""Pure-Python restatement of the scrub (include/wordpiece_amd_scrub.h), literal from the contract and byte by byte: the
classes, the e-mail at every '@', the IPv4 address of every NUM run, the hash that picks the placeholder, the signals, the
document rules and the three forms of the result.  No regular expression is used here; tests/test_scrub_model.py holds this
model against one."""
SIGNALS = ("bytes", "out_bytes", "at_signs", "emails", "email_bytes", "ips", "ip_bytes", "ips_left")
RULES = ("max_emails", "max_ips")
S = {name: k for k, name in enumerate(SIGNALS)}
EMAIL, IPV4, KEEP_PRIVATE = 1, 2, 4
AL = frozenset(range(65, 91)) | frozenset(range(97, 123))
AN = AL | frozenset(range(48, 58))
LOC, DOM, NUM = AN | frozenset(b"._%+-"), AN | frozenset(b".-"), frozenset(b"0123456789.")
PRIVATE = ((0, 8), (10 << 24, 8), (127 << 24, 8), (169 << 24 | 254 << 16, 16), (172 << 24 | 16 << 16, 12), (192 << 24 | 168 << 16, 16), (224 << 24, 3))
wordish = lambda b: b in AN or b == 95 or b >= 0x80  # noqa: E731
is_private = lambda address: any(address >> (32 - bits) == base >> (32 - bits) for base, bits in PRIVATE)  # noqa: E731


def emails(row):
    """-> [(start, end)] of the e-mail matches of one row, ascending"""
    out = []
    for p, b in enumerate(row):
        if b != 64:
            continue
        a = p
        while a > 0 and row[a - 1] in LOC:
            a -= 1
        if p - a > 64 or (a > 0 and row[a - 1] == 64):
            continue
        s = a
        while s < p and row[s] not in AN:
            s += 1
        e = p + 1
        while e < len(row) and row[e] in DOM:
            e += 1
        if s == p or e - (p + 1) > 255:
            continue
        at, end = p + 1, None
        for k, label in enumerate(bytes(row[p + 1:e]).split(b"."), 1):
            if not 1 <= len(label) <= 63 or label[0] == 45 or label[-1] == 45:
                break
            if k >= 2 and len(label) >= 2 and all(c in AL for c in label):
                end = at + len(label)
            at += len(label) + 1
        if end is not None:
            out.append((s, end))
    return out


def ipv4s(row):
    """-> [(start, end, address)] of the IPv4 matches of one row, ascending, those inside an e-mail included"""
    out, p, n = [], 0, len(row)
    while p < n:
        if row[p] not in NUM:
            p += 1
            continue
        e = p
        while e < n and row[e] in NUM:
            e += 1
        a, p = p, e
        if (a > 0 and wordish(row[a - 1])) or (e < n and wordish(row[e])) or e - a > 16:
            continue
        if row[e - 1] == 46:
            e -= 1
        parts = bytes(row[a:e]).split(b".")
        if len(parts) == 4 and all(1 <= len(d) <= 3 and int(d) <= 255 and (d == b"0" or d[0] != 48) for d in parts):
            out.append((a, e, int(parts[0]) << 24 | int(parts[1]) << 16 | int(parts[2]) << 8 | int(parts[3])))
    return out


def fnv1a(match):
    h = 2166136261
    for b in match:
        h = ((h ^ (b + 32 if 65 <= b <= 90 else b)) * 16777619) & 0xFFFFFFFF
    return h


def matches(row, kinds):
    """-> [(start, end, kind)] of one row in text order: 0 e-mail, 1 IPv4 replaced, 2 IPv4 left"""
    es = emails(row) if kinds & EMAIL else []
    out = [(s, e, 0) for s, e in es]
    for s, e, address in ipv4s(row) if kinds & IPV4 else []:
        if not any(a <= s and e <= b for a, b in es):
            out.append((s, e, 2 if kinds & KEEP_PRIVATE and is_private(address) else 1))
    return sorted(out)


def scrub_rows(data, off, kinds=EMAIL | IPV4, email_repl=(b"",), ip_repl=(b"",), rules=None):
    """The whole call over the batch (data, off) -> every array of every want bit, as lists and bytes, and "stats"."""
    data, n = bytes(data), len(off) - 1
    limit = [-1, -1]
    for name, value in dict(rules or {}).items():
        limit[RULES.index(name)] = int(value)
    sig = [[0] * n for _ in SIGNALS]
    reasons, out_rows = [], []
    m = dict(match_row=[], match_start=[], match_len=[], match_kind=[], match_repl=[])
    for r in range(n):
        row, at, new = data[off[r]:off[r + 1]], 0, b""
        sig[S["bytes"]][r], sig[S["at_signs"]][r] = len(row), row.count(b"@")
        for s, e, kind in matches(row, kinds):
            repl = (email_repl, ip_repl, None)[kind]
            pick = fnv1a(row[s:e]) % len(repl) if repl else -1
            new += row[at:s] + (row[s:e] if kind == 2 else bytes(repl[pick]))
            at = e
            for key, x in zip(m, (r, off[r] + s, e - s, kind, pick)):
                m[key].append(x)
            sig[S[("emails", "ips", "ips_left")[kind]]][r] += 1
            if kind < 2:
                sig[S[("email_bytes", "ip_bytes")[kind]]][r] += e - s
        new += row[at:]
        out_rows.append(new)
        sig[S["out_bytes"]][r] = len(new)
        bits = (limit[0] >= 0 and sig[S["emails"]][r] > limit[0]) | (limit[1] >= 0 and sig[S["ips"]][r] + sig[S["ips_left"]][r] > limit[1]) << 1
        reasons.append(int(bits))
    def ends(rows):  # (a running sum: a batch of 2,000 rows is a case of tests/scrub_edge_cases.py)
        out = [0]
        for x in rows:
            out.append(out[-1] + len(x))
        return out
    kept = [r for r in range(n) if reasons[r] == 0]
    stats = dict(n_rows=n, n_bytes=off[n] if n else 0, n_out_bytes=sum(map(len, out_rows)), n_matches=[m["match_kind"].count(k) for k in range(3)],
                 rule_failed=[sum(b >> k & 1 for b in reasons) for k in range(2)], n_kept=len(kept))
    return dict(m, signals=sig, reasons=reasons, out_data=b"".join(out_rows), out_off=ends(out_rows), kept=kept, data=b"".join(out_rows[r] for r in kept),
                row_off=ends([out_rows[r] for r in kept]), stats=stats)
