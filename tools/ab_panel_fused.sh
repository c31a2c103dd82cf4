# config C hot path alone, fused panel launches off / automatic (BGP_PANEL_FUSED=0 / unset), alternating three times on one box:
# ms per step (three timed passes each) and the kernel split.  Accepted when every automatic value lies below the lowest of the other side.
for rep in 1 2 3; do
  for v in 0 auto; do
    if [ $v = auto ]; then unset BGP_PANEL_FUSED; else export BGP_PANEL_FUSED=$v; fi
    echo -n "BGP_PANEL_FUSED=$v: "; python bench.py --full --no-extras --steps 20 --warmup 3 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read()); print([round(t,3) for t in d['timed_passes_ms_per_step']], {k: round(v,4) for k,v in d['kernel_ms_per_half_step'].items()}, round(d['roofline']['frac'],4))"
  done
done
