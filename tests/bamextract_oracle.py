"""BamExtract restated in Python (src/BamExtract/main.cpp:27-83), independent of the device: the ID file as :35-44 reads it, the sequential loop of :63-76 and the
log. A record's name is what BamAlignment::name() gives (src/cppNGS/BamReader.h:69-72, bam_get_qname as a C string): the bytes in front of the first NUL of the
l_read_name bytes. The record bytes are bamfilter_oracle.written's (BamWriter::writeAlignment)."""
from bamfilter_oracle import Rec, read_bam, written  # noqa: F401

BLANKS = b"\t\n\v\f\r "   # QByteArray::trimmed()


def parse_ids(data):
    """the set of read names of an ID file's bytes: lines split at \\n (a last line without one counts), trimmed at both ends, empty and '#' lines skipped"""
    ids = set()
    for line in data.split(b"\n"):
        line = line.strip(BLANKS)
        if line and line[:1] != b"#":
            ids.add(line)
    return ids


def name_of(rec_bytes):
    return rec_bytes[36:36 + rec_bytes[12]].split(b"\0", 1)[0]


def extract(records, ids, with_out2):
    """records: record bytes in file order. -> (records of out, records of out2, dict(out, out2, names))"""
    out, out2 = [], []
    for b in records:
        if name_of(b) in ids:
            out.append(written(Rec(b)))
        elif with_out2:
            out2.append(written(Rec(b)))
    return out, out2, dict(out=len(out), out2=len(out2), names=len(ids))


def log_text(counts, with_out2):
    t = "Read IDs: %d\nReads written to 'out': %d\n" % (counts["names"], counts["out"])
    return t + ("Reads written to 'out2': %d\n" % counts["out2"] if with_out2 else "")
