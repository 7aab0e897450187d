"""Summarise `hipcc -Rpass-analysis=kernel-resource-usage` output per pass kernel (P, T)."""
import re
import sys

txt = open(sys.argv[1]).read()
tmin = int(sys.argv[2]) if len(sys.argv) > 2 else 0
OCC = r"Occupancy \[waves/SIMD\]"
for p in re.split(r"remark: Function Name: ", txt)[1:]:
    name = p.split()[0]
    # (pass_kernel_repair / _select / _verify have no narrow variant: two template arguments)
    m = re.match(r"_ZN4rs16\d+pass_kernel(_late(?:_paired|_tower)?|_repair|_select|_verify)?ILi(\d+)ELi(\d+)E(?:Li(\d+)E)?"
                 r"(?:Lb([01])ELb([01])E)?", name)
    if not m or int(m.group(3)) < tmin:
        continue
    late = {None: "", "_late": " late", "_late_paired": " late", "_late_tower": " late tower", "_repair": " repair",
            "_select": " select", "_verify": " verify"}[m.group(1)]
    if m.group(5):  # the paired-rows flavours: which sides are paired
        late += " paired " + "+".join(s for s, on in (("in", m.group(5)), ("out", m.group(6))) if on == "1")

    def g(k):
        mm = re.search(k + r": (\d+)", p)
        return mm.group(1) if mm else "?"

    print("P%s T%s NV%s%s  VGPR %s  SGPR %s  occ %s  sspill %s  vspill %s  scratch %s  LDS %s" % (
        m.group(2), m.group(3), m.group(4) or "0", late, g("VGPRs"), g("SGPRs"), g(OCC), g("SGPRs Spill"), g("VGPRs Spill"),
        g(r"ScratchSize \[bytes/lane\]"), g(r"LDS Size \[bytes/block\]")))
