"""Resource-usage table of the render kernel's instantiations, one commit against another.

    hipcc <build.py's HIP_FLAGS> --cuda-device-only -Rpass-analysis=kernel-resource-usage \
          -c gp1_raytracer_2223_amd/csrc/rtx_hip.hip -o /dev/null 2> usage.log      (once per commit)
    python tools/resource_table.py parent_usage.log this_usage.log

Instantiations are matched by their template arguments (a trailing SS = false is the plain kernel);
the SS variants, which only the second log has, are listed beside their plain twins."""
import re, sys, subprocess
def parse(path):
    out = {}; cur = None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m: cur = m.group(1); out[cur] = {}; continue
        m = re.search(r":\s+([A-Za-z /\[\]]+?): (\S+) \[-Rpass", line)
        if m and cur: out[cur][m.group(1).strip()] = m.group(2)
    return out
def key(n):
    m = re.search(r"rtx_render_kernelILb(\d)ELi(\d)ELb(\d)ELi(\d+)ELb(\d)ELb(\d)E(?:Lb(\d)E)?", n)
    if not m: return n
    g = m.groups()
    return "COUNT=%s PHASE=%s DEEP=%s SPEC=%s HSTK=%s CULLK=%s" % g[:6] + (" SS=1" if g[6] == "1" else "")
a, b = parse(sys.argv[1]), parse(sys.argv[2])
a = {key(k): v for k, v in a.items()}; b = {key(k): v for k, v in b.items()}
keys = ["TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]
short = ["SGPR", "VGPR", "scratch", "occ", "sspill", "vspill", "LDS"]
names = [n for n in a if n.startswith("COUNT=")]
def tmpl(n): return n
print("%-58s %s   (parent -> this commit; '=' unchanged)" % ("rtx_render_kernel<...>", " ".join("%-9s" % s for s in short)))
diff = 0
for n in names:
    cells = []
    for k in keys:
        x, y = a[n].get(k), b.get(n, {}).get(k)
        if x == y: cells.append("%-9s" % (x + " ="))
        else: cells.append("%-9s" % ("%s->%s" % (x, y))); diff += 1
    print("%-58s %s" % (tmpl(n), " ".join(cells)))
print("instantiations: %d, cells that differ: %d" % (len(names), diff))
others = [n for n in a if not n.startswith("COUNT=") and a[n] != b.get(n)]
print("other kernels of the file that differ:", others if others else "none")

new = [n for n in b if n.endswith("SS=1")]
print()
print("the new SS instantiations (this commit only) against their plain twin:")
for n in new:
    t = n[:-5]
    print("%-58s %s" % (n, " ".join("%-9s" % ("%s (%s)" % (b[n].get(k), b[t].get(k))) for k in keys)))
