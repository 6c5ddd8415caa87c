#!/usr/bin/env python3
"""tests/golden/vectors/wide_subjects.json: what the REAL reference makes of
the input of tests/wide_cases.py -- three samples, 1 310 000 distinct
subjects, `woltka classify --rank none,genus` -- (build container only; the
input is regenerated from its seed; the tables are too large to commit, so
the sha256, the row count and the first and last ten rows of each are kept).

    python tests/golden/make_wide_reference.py
"""
import contextlib
import io
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import wide_cases as W  # noqa: E402

OUT = os.path.join(HERE, 'vectors', 'wide_subjects.json')


def main():
    import _refshim
    if not _refshim.install():
        sys.exit('the reference tree is not here')
    from click.testing import CliRunner
    from woltka.cli import cli
    with tempfile.TemporaryDirectory() as tmp:
        args = W.write_inputs(tmp, 'map')
        out = os.path.join(tmp, 'out')
        with contextlib.redirect_stdout(io.StringIO()):
            res = CliRunner().invoke(cli, ['classify'] + args + ['--output', out])
        if res.exit_code != 0:
            sys.exit(f'the reference failed: {res.output}\n{res.exception!r}')
        tables = W.digests(out)
    for fn, d in tables.items():
        print(fn, d['rows'], d['sha256'])
    doc = {'seed': W.SEED, 'n_subjects': W.N_SUBJECTS, 'samples': W.SAMPLES,
           'args': W.ARGS, 'tables': tables}
    with open(OUT, 'w') as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
