#!/usr/bin/env python3
"""Pin the host dispatch of csrc/gemm.hip beyond the BASELINE shapes: every unique row of tests/golden/dispatch_table.json that one of
gemm.hip's nine entry points serves is replayed as a DRY RUN (segmentation_factory_amd/dispatch.py: placeholder pointers, nothing
launched, no GPU needed) under one perturbation at a time -- every policy switch of the GEMM / implicit-GEMM sections of csrc/policy.h
flipped, operand alignment, leading dimensions, slice counts, the membership of grouped calls -- and the host queries that size
workspaces and choose slice counts are recorded over the distinct shapes of those rows.

    python tools/make_gemm_dispatch_sweep.py [--out tests/golden/gemm_dispatch_sweep.json]
    SEGFAC_HIP_LIB=/path/to/another/libsegfac_hip.so python tools/make_gemm_dispatch_sweep.py --out /tmp/other.json

Two builds whose host dispatch agrees write identical bytes.  tests/test_host_cpu.py::test_gemm_dispatch_sweep regenerates the sweep in
memory and compares it with the committed file.  A return code other than 0 is a recorded result like any other.

File layout: 'kernels' = the distinct kernel names; 'results' = the distinct results, [return code, kernel, kernel, ...]; 'base' = one
result (index) per row (rows = `rows(table)` below, pinned by 'rows_sha256'); 'perturbed' = per perturbation only the rows whose result
differs from 'base', as a flat [row, result, row, result, ...], or '= <name>' where an earlier perturbation has the same list; 'queries'
the same way for the host queries over the sorted distinct shapes.  `explain()` decodes it."""
import argparse
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
# entry point -> (index of the output pointer, indices of the leading dimensions, index of split_k or None, index of ws or None)
ENTRY = {
    'segf_gemm': (9, (6, 8, 11, 14), 17, 18),
    'segf_gemm_dw_db': (8, (5, 7, 10), 11, 12),
    'segf_gemm_pro': (9, (6, 8, 11), 13, 14),
    'segf_conv3x3': (10, (7, 9, 12), 14, 15),
    'segf_conv3x3_fp8': (12, (7, 10, 13), None, None),
    'segf_conv3x3_fp8_wgrad': (11, (6, 9, 12), 13, 14),
    'segf_linear_fp8': (10, (5, 8, 11, 14), None, None),
    'segf_linear_fp8_wgrad': (9, (4, 7, 10), 11, 12),
    'segf_gemm_dw_db_grouped': None,
}
# numeric switches: one value well below and one well above the default (g8_stagger: its two explicit settings)
THRESHOLDS = {'gemm8_linear_min_tiles': (16, 1024), 'gemm8_linear_min_fill': (10, 95), 'gemm8_linear_min_k': (64, 2048),
              'gemm8_dw_min_gflop': (1, 10000), 'gemm8_linear_min_gflop': (1, 10000), 'g8_stagger': (0, 1)}
SECTIONS = ('GEMM family', 'implicit-GEMM')


def switches():
    """[(field, value)] : every switch of the two sections of csrc/policy.h, off its default."""
    text = open(os.path.join(ROOT, 'segmentation_factory_amd', 'csrc', 'policy.h')).read()
    out, on = [], False
    for line in text.splitlines():
        m = re.search(r'/\* ---- (.*?) ---- \*/', line)
        if m:
            on = m.group(1).startswith(SECTIONS)
            continue
        m = re.match(r'\s*X\((\w+), "SEGFAC_\w+", (-?\d+),', line)
        if m and on:
            field, default = m.group(1), int(m.group(2))
            if field in THRESHOLDS:
                out += [(field, v) for v in THRESHOLDS[field]]
            else:
                assert default in (0, 1), (field, default)
                out.append((field, 1 - default))
    assert len({f for f, _ in out}) == 33, out          # 24 + 9 rows of the two sections
    return out


def rows(table):
    """Unique (entry point, arguments) rows of the dispatch table that gemm.hip serves, in order of first appearance."""
    seen, out = set(), []
    for entries in table.values():
        for e in entries:
            key = (e['fn'], repr(e['args']))
            if e['fn'] in ENTRY and key not in seen:
                seen.add(key)
                out.append({'fn': e['fn'], 'args': e['args']})
    return out


def _mnk(row):
    """(M, N, K) of the product a row computes, as segf_gemm_pick_splitk takes them (None for the grouped rows)."""
    fn, a = row['fn'], row['args']
    if fn in ('segf_gemm', 'segf_gemm_pro'):
        return a[2], a[3], a[4]
    if fn == 'segf_gemm_dw_db':
        return a[1], a[2], a[3]
    if fn == 'segf_linear_fp8':
        return a[1], a[2], a[3]
    if fn == 'segf_linear_fp8_wgrad':
        return a[0], a[1], a[2]
    if fn == 'segf_conv3x3':
        mode, B, H, W, Cin, Cout = a[:6]
        P = B * H * W
        return (Cout, 9 * Cin, P) if mode == 2 else (P, Cout if mode == 0 else Cin, 9 * (Cin if mode == 0 else Cout))
    if fn == 'segf_conv3x3_fp8_wgrad':
        B, H, W, Cin, Cout = a[:5]
        return Cout, 9 * Cin, B * H * W
    return None


def _conv(row):
    fn, a = row['fn'], row['args']
    if fn in ('segf_conv3x3', 'segf_conv3x3_fp8'):
        return tuple(a[1:6])
    if fn == 'segf_conv3x3_fp8_wgrad':
        return tuple(a[:5])
    return None


def _with(row, edits):
    args = list(row['args'])
    for i, v in edits.items():
        args[i] = v
    return {'fn': row['fn'], 'args': args}


def _is_ptr(v):
    return isinstance(v, str) and v.startswith('p')


def perturbations(lib):
    """[(name, function row -> (row, low bits of the grouped pointers) or None when the perturbation does not apply)]"""
    def align_all(bits):
        def f(row):
            if row['fn'] == 'segf_gemm_dw_db_grouped':
                return row, (bits,) * 5
            return _with(row, {i: 'p%d' % bits for i, v in enumerate(row['args']) if _is_ptr(v)}), None
        return f

    def align_out(row):
        if row['fn'] == 'segf_gemm_dw_db_grouped':
            return row, (0, 0, 8, 0, 0)
        return _with(row, {ENTRY[row['fn']][0]: 'p8'}), None

    def ld_plus_one(row):
        if row['fn'] == 'segf_gemm_dw_db_grouped':
            dt, desc = row['args']
            return {'fn': row['fn'], 'args': [dt, [m[:3] + [v + 1 if v > 0 and v % 8 == 0 else v for v in m[3:6]] + m[6:] for m in desc]]}, None
        return _with(row, {i: row['args'][i] + 1 for i in ENTRY[row['fn']][1] if row['args'][i] > 0 and row['args'][i] % 8 == 0}), None

    def split(how):
        def value(rec, mnk):
            if how == 'pick':
                return lib.segf_gemm_pick_splitk(*mnk)
            return 1 if how == 'one' else max(rec + how, 0)

        def f(row):
            if row['fn'] == 'segf_gemm_dw_db_grouped':
                dt, desc = row['args']
                return {'fn': row['fn'], 'args': [dt, [m[:6] + [value(m[6], m[:3]), m[7]] for m in desc]]}, None
            sk, ws = ENTRY[row['fn']][2:]
            if sk is None:
                return None
            edits = {sk: value(row['args'][sk], _mnk(row))}
            if row['args'][ws] is None:
                edits[ws] = 'p0'                  # (so that the route is exercised, not only the missing-workspace error)
            return _with(row, edits), None
        return f

    def grouped(edit):
        def f(row):
            if row['fn'] != 'segf_gemm_dw_db_grouped':
                return None
            dt, desc = row['args']
            return {'fn': row['fn'], 'args': [dt, edit(desc)]}, None
        return f

    return [('align:all_p8', align_all(8)), ('align:out_p8', align_out), ('align:all_p2', align_all(2)), ('ld:+1', ld_plus_one),
            ('split:1', split('one')), ('split:-1', split(-1)), ('split:+1', split(1)), ('split:pick', split('pick')),
            ('group:shared_split flipped', grouped(lambda d: [m[:7] + [1 - m[7]] for m in d])),
            ('group:reversed', grouped(lambda d: d[::-1])),
            ('group:first alone', grouped(lambda d: d[:1])),
            ('group:13 copies of the first', grouped(lambda d: [d[0]] * 13))]


def queries(lib, mnk, conv):
    """{query: [answers over the shapes]}"""
    q = {}
    pick = [lib.segf_gemm_pick_splitk(*s) for s in mnk]
    q['segf_gemm_pick_splitk'] = pick
    q['segf_gemm_dw_db_ws(split_k=pick)'] = [lib.segf_gemm_dw_db_ws(*s, p) for s, p in zip(mnk, pick)]
    for layout in (0, 2):
        q[f'segf_gemm_pro_supported(layout={layout},rpg=256)'] = [lib.segf_gemm_pro_supported(1, layout, *s, 256) for s in mnk]
    for mode in (0, 1, 2):
        q[f'segf_linear_fp8_supported(mode={mode})'] = [lib.segf_linear_fp8_supported(mode, *s) for s in mnk]
    q['segf_linear_fp8_wgrad_splitk'] = [lib.segf_linear_fp8_wgrad_splitk(*s) for s in mnk]
    q['segf_conv3x3_pick_splitk'] = [lib.segf_conv3x3_pick_splitk(Cin, Cout, B * H * W) for B, H, W, Cin, Cout in conv]
    for mode in (0, 1):
        q[f'segf_conv3x3_fwd_splitk(mode={mode})'] = [lib.segf_conv3x3_fwd_splitk(mode, *s) for s in conv]
        q[f'segf_conv3x3_fp8_supported(mode={mode})'] = [lib.segf_conv3x3_fp8_supported(mode, *s) for s in conv]
    q['segf_conv3x3_fp8_wgrad_supported'] = [lib.segf_conv3x3_fp8_wgrad_supported(*s) for s in conv]
    return q


def generate(table=None):
    from segmentation_factory_amd import dispatch, hip
    if table is None:
        with open(os.path.join(GOLDEN, 'dispatch_table.json')) as fh:
            table = json.load(fh)
    lib = hip.lib()
    rs = rows(table)
    names, results, index = [], [], {}

    def run(row, low=None):
        rc, kernels = dispatch.replay_rc(row, low or (0, 0, 0, 0, 0))
        key = (rc, tuple(kernels))
        if key not in index:
            for k in kernels:
                if k not in names:
                    names.append(k)
            index[key] = len(results)
            results.append([rc] + [names.index(k) for k in kernels])
        return index[key]

    def same_as(diff, earlier):
        return next(('= ' + k for k, v in earlier.items() if v == diff), diff)

    base = [run(r) for r in rs]
    perturbed, n_results = {}, len(base)

    def sweep(name, f):
        nonlocal n_results
        diff = []
        for i, r in enumerate(rs):
            pr = f(r)
            if pr is None:
                continue
            n_results += 1
            got = run(*pr)
            if got != base[i]:
                diff += [i, got]
        perturbed[name] = same_as(diff, perturbed)

    sw = switches()
    for field, value in sw:
        with hip.policy_override(**{field: value}):
            sweep(f'policy:{field}={value}', lambda r: (r, None))
    for name, f in perturbations(lib):
        sweep(name, f)

    mnk = sorted({tuple(m[:3]) for r in rs if r['fn'] == 'segf_gemm_dw_db_grouped' for m in r['args'][1]} |
                 {_mnk(r) for r in rs if _mnk(r)})
    conv = sorted({_conv(r) for r in rs if _conv(r)})
    qbase = queries(lib, mnk, conv)
    n_queries = sum(len(v) for v in qbase.values())
    qpert = {}
    for field, value in sw:
        with hip.policy_override(**{field: value}):
            got = queries(lib, mnk, conv)
        n_queries += sum(len(v) for v in got.values())
        diff = {k: [x for i, (v, b) in enumerate(zip(got[k], qbase[k])) if v != b for x in (i, v)] for k in got if got[k] != qbase[k]}
        qpert[f'policy:{field}={value}'] = same_as(diff, qpert)
    return {'rows_sha256': hashlib.sha256(json.dumps(rs, separators=(',', ':')).encode()).hexdigest(), 'n_rows': len(rs),
            'n_results': n_results, 'n_query_results': n_queries, 'kernels': names, 'results': results, 'base': base,
            'perturbed': perturbed, 'queries': {'n_mnk': len(mnk), 'n_conv': len(conv), 'base': qbase, 'perturbed': qpert}}


def explain(sweep):
    """{perturbation: {row: (return code, kernel names)}} with 'unperturbed' = every row (for reading a mismatch)."""
    def named(r):
        return sweep['results'][r][0], [sweep['kernels'][k] for k in sweep['results'][r][1:]]
    out = {'unperturbed': {i: named(r) for i, r in enumerate(sweep['base'])}}
    for name, d in sweep['perturbed'].items():
        d = sweep['perturbed'][d[2:]] if isinstance(d, str) else d
        out[name] = {i: named(r) for i, r in zip(d[::2], d[1::2])}
    return out


def dumps(sweep):
    """One line per perturbation (diffs of a regenerated file stay readable)."""
    def one(v):
        return json.dumps(v, separators=(',', ':'), sort_keys=True)

    def block(d):
        return '{\n' + ',\n'.join(f'{json.dumps(k)}:{one(v)}' for k, v in d.items()) + '\n}'
    top = []
    for k, v in sweep.items():
        if k == 'perturbed':
            top.append(f'"{k}":{block(v)}')
        elif k == 'queries':
            top.append(f'"{k}":{{\n' + ',\n'.join(f'"{kk}":{block(vv) if kk == "perturbed" else one(vv)}' for kk, vv in v.items()) + '\n}')
        else:
            top.append(f'"{k}":{one(v)}')
    return '{\n' + ',\n'.join(top) + '\n}\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(GOLDEN, 'gemm_dispatch_sweep.json'))
    a = ap.parse_args()
    sweep = generate()
    text = dumps(sweep)
    assert json.loads(text) == sweep
    with open(a.out, 'w') as fh:
        fh.write(text)
    print(f"written {a.out}: {len(text)} bytes, {sweep['n_rows']} rows, {sweep['n_results']} (row, perturbation) results, "
          f"{sweep['n_query_results']} query results, {len(sweep['results'])} distinct results")


if __name__ == '__main__':
    main()
