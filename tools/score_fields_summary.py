"""`pytest -s -k score_fields` output (one `score-field <tier> <case>: err .. E32 .. bound ..` line per case) -> the two files of
profiles/attention_score_fields/ that stand for it:

    python tools/score_fields_summary.py device_full.log --json > score_fields.json
        per entry point and field class: cases, largest err, largest E32, largest err / bound, largest err / E32 (over the
        cases whose 2 E32 is above the floor: below it the floor decides); every case beyond half of its bound in full
    python tools/score_fields_summary.py device_full.log --log > device.log
        the log itself with the cases of one launch configuration folded into one line (cases, largest err, E32, err / bound
        and the case that has it); cases beyond a quarter of their bound and everything that is no case line stay as printed"""
import json
import re
import sys

LINE = re.compile(r'score-field (\w+) (.*): err (\S+) E32 (\S+) bound (\S+?)(\s+<-- FAIL)?$')
FIELD = re.compile(r' ((?:uniform|stair_\w+|straddle|ramp|spike|level|cold_but_last_tile_hot|relpos)\S*( h\d)?( known-answer)?)$')


def split_case(case):
    """(launch configuration, field) of a case name"""
    m = FIELD.search(case)
    if m:
        return case[:m.start()], m.group(1)
    m = re.match(r'(sam_t2i_fold R=\d+ N=\d+ T=\d+) (.*)', case)
    return (m.group(1), m.group(2)) if m else (case, '')


def field_class(field):
    cls = re.match(r'[a-z_]+', field).group(0) if field else 'other'
    if field.startswith('amp='):
        cls = 'amplitude / offset'
    return cls + ('/divergent' if '/' in field else '') + (' known-answer' if 'known-answer' in field else '')


def parse(path):
    for line in open(path):
        line = line.rstrip('\n')
        m = LINE.search(line.lstrip('.'))
        yield (line, None) if not m else (line, (m.group(2), float(m.group(3)), float(m.group(4)), float(m.group(5)), bool(m.group(6))))


def to_json(path):
    groups, close, n, over = {}, [], 0, 0
    for _, c in parse(path):
        if c is None:
            continue
        case, err, e32, bound, fail = c
        tag, field = split_case(case)
        n, over = n + 1, over + fail
        g = groups.setdefault(f'{tag.split(" ")[0]} | {field_class(field)}', dict(cases=0, max_err=0.0, max_E32=0.0, max_err_over_bound=0.0,
                                                                               max_err_over_E32=None))
        g['cases'] += 1
        g['max_err'], g['max_E32'] = max(g['max_err'], err), max(g['max_E32'], e32)
        g['max_err_over_bound'] = max(g['max_err_over_bound'], round(err / bound, 3))
        if 2.0 * e32 >= bound and e32 > 0:
            g['max_err_over_E32'] = max(g['max_err_over_E32'] or 0.0, round(err / e32, 3))
        if err > 0.5 * bound:
            close.append(dict(case=case, err=err, E32=e32, bound=bound))
    rows = lambda d: ',\n'.join(f'  {json.dumps(k)}: {json.dumps(v)}' for k, v in d.items())
    print('{\n "cases": %d, "over_the_bound": %d, "bound": "max(F, 2 E32)",\n "groups": {\n%s\n },\n "beyond_half_of_the_bound": [\n%s\n ]\n}'
          % (n, over, rows(groups), ',\n'.join('  ' + json.dumps(c) for c in close)))


def to_log(path):
    cur, acc = None, []

    def flush():
        if acc:
            w = max(acc, key=lambda a: a[1] / a[3])
            print(f'score-field {cur}: {len(acc)} cases within a quarter of their bound, max err {max(a[1] for a in acc):.3e}, '
                  f'max E32 {max(a[2] for a in acc):.3e}, max err / bound {w[1] / w[3]:.3f} ({w[0]})')
        acc.clear()
    for line, c in parse(path):
        tag = split_case(c[0])[0] if c else None
        if tag != cur:
            flush()
            cur = tag
        if c is None or c[4] or c[1] > 0.25 * c[3]:
            print(line)
        else:
            acc.append((split_case(c[0])[1],) + c[1:4])
    flush()


if __name__ == '__main__':
    (to_json if '--json' in sys.argv else to_log)(sys.argv[1])
