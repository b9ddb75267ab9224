#!/bin/bash
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=gpurun_out/pmc_occ
mkdir -p $OUT
rocprofv3 --kernel-trace --pmc SQ_LEVEL_WAVES SQ_CYCLES SQ_BUSY_CYCLES SQ_WAVES SQ_WAVE_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT -o occ -- python3 bench.py --steps 4 --warmup 6 --no-cpu-baseline > $OUT/occ.log 2>&1 || { tail -5 $OUT/occ.log; exit 1; }
python3 - <<'PY'
import csv, collections
rows=list(csv.DictReader(open('gpurun_out/pmc_occ/occ_counter_collection.csv')))
acc=collections.defaultdict(lambda: collections.defaultdict(list))
res={}
for r in rows:
    k=r['Kernel_Name'].split('(')[0][-70:]
    acc[k][r['Counter_Name']].append(float(r['Counter_Value']))
    res[k]=(r.get('LDS_Block_Size'), r.get('VGPR_Count'), r.get('Accum_VGPR_Count'), r.get('SGPR_Count'), r.get('Grid_Size'), r.get('Workgroup_Size'))
for k,d in acc.items():
    for cn,v in d.items(): print(f"{k:42s} {cn:16s}", sum(v[-4:])/len(v[-4:]))
    print(k, 'LDS %s VGPR %s AGPR %s SGPR %s grid %s wg %s' % res[k])
PY
