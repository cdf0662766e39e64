"""tools/kernel_coverage.py on a synthetic device-assembly snippet and synthetic rocprofv3 CSVs written here.  No GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
kc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kc)

ASM = """\
\t.text
\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.protected\t_Z5alphaILi4EEvPf
\t.globl\t_Z5alphaILi4EEvPf
_Z5alphaILi4EEvPf:
\tv_mov_b32_e32 v0, 0        ; a comment that says .amdhsa_kernel _Z4fakev in passing
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _Z5alphaILi4EEvPf
\t\t.amdhsa_group_segment_fixed_size 0
\t.end_amdhsa_kernel
\t.amdhsa_kernel _Z5alphaILi8EEvPf
\t.end_amdhsa_kernel
    .amdhsa_kernel _Z4betav
\t.end_amdhsa_kernel
amdhsa.kernels:
  - .name:           _Z5gammav
"""
TRACE = '''"Kind","Agent_Id","Queue_Id","Kernel_Id","Kernel_Name","Correlation_Id","Start_Timestamp","End_Timestamp"
"KERNEL_DISPATCH","Agent 2",1,7,"__amd_rocclr_copyBuffer.kd",1,10,20
"KERNEL_DISPATCH","Agent 2",1,8,"_Z5alphaILi4EEvPf.kd",2,30,40
"KERNEL_DISPATCH","Agent 2",1,8,"_Z5alphaILi4EEvPf.kd",3,50,60
'''
STATS = '''"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"
"_Z4betav.kd",31,979,31.5,11.06,5,34,4.8
"_ZN2at6native6kernelIfEEvT_.kd",2,86,34.5,9.77,5,90,2.0
'''


def test_asm_parser_reads_only_the_kernel_directive_lines():
    assert kc.parse_asm(ASM) == ["_Z5alphaILi4EEvPf", "_Z5alphaILi8EEvPf", "_Z4betav"]
    assert kc.parse_asm("") == [] and kc.parse_asm("\t.end_amdhsa_kernel\n") == []


def test_csv_parser_takes_traces_and_statistics():
    assert kc.parse_csv(TRACE) == {"__amd_rocclr_copyBuffer": 1, "_Z5alphaILi4EEvPf": 2}
    assert kc.parse_csv(STATS) == {"_Z4betav": 31, "_ZN2at6native6kernelIfEEvT_": 2}
    assert kc.parse_csv("") == {} and kc.parse_csv('"Domain","Calls"\n"KERNEL_DISPATCH",3\n') == {}


def test_record_accounts_for_every_instance(tmp_path):
    asm, base, now = tmp_path / "build", tmp_path / "base", tmp_path / "now"
    for d in (asm, base / "grp_a", now / "grp_b"):
        d.mkdir(parents=True)
    (asm / "one.s").write_text(ASM)
    (asm / "host_only.s").write_text("\t.text\n")
    (base / "grp_a" / "1_kernel_trace.csv").write_text(TRACE)
    (now / "grp_b" / "9_kernel_stats.csv").write_text(STATS)
    groups = tmp_path / "groups.txt"
    groups.write_text("grp_a tests/test_a_gpu.py\ngrp_b tests/test_b_gpu.py tests/test_c_gpu.py\n")
    reasons = tmp_path / "reasons.txt"
    reasons.write_text("# regex <TAB> reason\nalpha<8>\tunreachable through the C ABI: host.hip:12 never selects 8\n")
    ship = kc.shipped(str(asm))
    assert ship == {"one.hip": ["_Z5alphaILi4EEvPf", "_Z5alphaILi8EEvPf", "_Z4betav"]}
    before, after = kc.launched(str(base)), kc.launched(str(now))
    assert kc.coverage(ship, before) == {"_Z5alphaILi4EEvPf": "grp_a"}
    text, unaccounted = kc.report(ship, before, after, kc.read_groups(str(groups)), kc.read_reasons(str(reasons)), "commit abc")
    assert unaccounted == 0
    assert text.startswith("commit abc\n") and "shipped instances: 3 in 1 device files" in text
    assert "before: 1    after: 2    not launched: 1" in text
    assert "<- tests/test_a_gpu.py" in text and "<- new: tests/test_b_gpu.py tests/test_c_gpu.py" in text
    assert "never selects 8" in text and "UNACCOUNTED" not in text
    text, unaccounted = kc.report(ship, before, after, {}, [], "")
    assert unaccounted == 1 and "UNACCOUNTED" in text
    out = tmp_path / "record.txt"
    rc = kc.main(["--asm", str(asm), "--baseline", str(base), "--traces", str(now), "--groups", str(groups),
                  "--reasons", str(reasons), "-o", str(out)])
    assert rc == 0 and "not launched: 1" in out.read_text()
