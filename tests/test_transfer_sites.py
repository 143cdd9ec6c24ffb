"""Every copy between host and device memory in tracer_amd/csrc names one of the context's three pinned buffers as its host side:
h_xfer (trc_copy_to_host / trc_copy_to_device / trc_read_to_host: every synchronous transfer), h_readback (the two asynchronous
read-backs: refit_run, sah_build_topology) or h_stage (host-staged collectives).  No copy hands the HIP runtime pageable memory
(DESIGN.md section 6 says why).  A scan of the sources: no GPU needed."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tracer_amd", "csrc")
PINNED = ("h_xfer", "h_readback", "h_stage")


def host_device_copies(text):
    """(line, call) of every hipMemcpy / hipMemcpyAsync call whose kind is host-to-device or device-to-host, each up to its `;`"""
    for m in re.finditer(r"\bhipMemcpy(?:Async)?\s*\(", text):
        call = text[m.start():text.index(";", m.end())]
        if re.search(r"\bhipMemcpy(?:HostToDevice|DeviceToHost)\b", call):
            yield text.count("\n", 0, m.start()) + 1, " ".join(call.split())


def unpinned_sites(csrc=CSRC):
    sites = []
    for path in sorted(p for ext in ("hip", "hpp", "inc") for p in glob.glob(os.path.join(csrc, "*." + ext))):
        for line, call in host_device_copies(open(path).read()):
            if not any(re.search(r"\b" + name + r"\b", call) for name in PINNED):
                sites.append(f"{os.path.basename(path)}:{line}: {call}")
    return sites


def test_the_scan_sees_the_copies():
    text = "a;\nHIP_TRY(ctx, hipMemcpyAsync(d, &h,\n   4, hipMemcpyHostToDevice, st));\nhipMemcpy(a, b, 4, hipMemcpyDeviceToDevice);\n"
    assert list(host_device_copies(text)) == [(2, "hipMemcpyAsync(d, &h, 4, hipMemcpyHostToDevice, st))")]
    assert sum(1 for p in glob.glob(os.path.join(CSRC, "*.hip")) for _ in host_device_copies(open(p).read())) >= 6


def test_every_host_device_copy_goes_through_a_pinned_buffer():
    sites = unpinned_sites()
    assert not sites, "copies that hand the runtime a host pointer of their own:\n" + "\n".join(sites)
