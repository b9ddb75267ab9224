#!/bin/bash
# Device assembly of one kernel of the library: tools/dis_kernel.sh <mangled-name-substring> [out.s]
# (every unit's assembly goes to /tmp/dis/<unit>.s, with smcnuts_amd/build.py's flags plus ${SMCN_DEFS})
set -e
cd "$(dirname "$0")/.."
python3 -m smcnuts_amd.build --asm /tmp/dis ${SMCN_DEFS} > /dev/null
python3 - "$1" "${2:-/tmp/dis/kernel.s}" <<'PY'
import glob, sys, re
pat = sys.argv[1]
for f in sorted(glob.glob('/tmp/dis/smcn_*.s')):
    s = open(f).read()
    m = re.search(r'^(\S*' + re.escape(pat) + r'[^\s:]*):', s, re.M)
    if m:
        break
i = m.start(); j = s.index('.Lfunc_end', i)
open(sys.argv[2], 'w').write(s[i:j])
print(m.group(1), s[i:j].count('\n'), 'lines ->', sys.argv[2], '(' + f + ')')
PY
