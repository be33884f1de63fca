# On the GPU box: pipelined step time against the number of batches in flight, two passes (LIB=<name> selects nim-blscurve_amd/variants/<name>.so)
cd $GRAFT_REPO_ROOT
[ -n "$LIB" ] && export MI355_BLS_LIB=$GRAFT_REPO_ROOT/nim-blscurve_amd/variants/$LIB.so
for pass in 1 2; do
for inflight in 3 2 4; do
  echo -n "inflight=$inflight  "
  python3 bench.py --steps 30 --warmup 4 --no-cpu --no-aux --no-one-caller --inflight $inflight 2>/dev/null | python3 -c "import sys,json; print(round(json.loads(sys.stdin.readline())['ms_per_step'],3))"
done; done
