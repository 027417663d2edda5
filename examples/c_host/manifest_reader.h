/* Reader of manifest.txt, the flat twin of manifest.json that pipe.export_call writes (reflecting_reality_amd/program.py::write_manifest):
 * one `key value` line per setting — nested keys joined by dots ("files.step step.mfprog", "io.conditioning.cond.shape 2,5,8,8"), lists
 * by commas, booleans as 0 / 1.  Plain C, no allocation, no dependency: inpaint_host.c includes it, and tests/test_program_call_cpu.py
 * builds it into a stand-alone program to check that what the exporter writes is what this reads. */
#ifndef MF_MANIFEST_READER_H
#define MF_MANIFEST_READER_H

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MF_MANIFEST_MAX_ENTRIES 256
#define MF_MANIFEST_KEY 96
#define MF_MANIFEST_VALUE 256

typedef struct mf_manifest_entry { char key[MF_MANIFEST_KEY]; char value[MF_MANIFEST_VALUE]; } mf_manifest_entry;
typedef struct mf_manifest { int n; mf_manifest_entry e[MF_MANIFEST_MAX_ENTRIES]; } mf_manifest;

/* 0 on success; otherwise -1 with a message in err (a missing file, a line without a value, a key or value that does not fit) */
static int mf_manifest_read(const char* path, mf_manifest* m, char* err, size_t errlen) {
    char line[MF_MANIFEST_KEY + MF_MANIFEST_VALUE + 8];
    FILE* f = fopen(path, "r");
    int lineno = 0;
    m->n = 0;
    if (!f) { snprintf(err, errlen, "%s: cannot open", path); return -1; }
    while (fgets(line, (int)sizeof(line), f)) {
        size_t len = strlen(line);
        char* sp;
        ++lineno;
        if (len && line[len - 1] == '\n') line[--len] = 0;
        else if (len + 1 == sizeof(line)) { snprintf(err, errlen, "%s:%d: line too long", path, lineno); fclose(f); return -1; }
        if (len && line[len - 1] == '\r') line[--len] = 0;
        if (!len) continue;
        sp = strchr(line, ' ');
        if (!sp || sp == line || !sp[1]) { snprintf(err, errlen, "%s:%d: expected `key value`", path, lineno); fclose(f); return -1; }
        if ((size_t)(sp - line) >= MF_MANIFEST_KEY || strlen(sp + 1) >= MF_MANIFEST_VALUE) {
            snprintf(err, errlen, "%s:%d: key or value too long", path, lineno);
            fclose(f);
            return -1;
        }
        if (m->n == MF_MANIFEST_MAX_ENTRIES) { snprintf(err, errlen, "%s: more than %d entries", path, MF_MANIFEST_MAX_ENTRIES); fclose(f); return -1; }
        memcpy(m->e[m->n].key, line, (size_t)(sp - line));
        m->e[m->n].key[sp - line] = 0;
        strcpy(m->e[m->n].value, sp + 1);
        ++m->n;
    }
    fclose(f);
    return 0;
}

/* the value of a key, or NULL */
static const char* mf_manifest_get(const mf_manifest* m, const char* key) {
    int i;
    for (i = 0; i < m->n; ++i)
        if (!strcmp(m->e[i].key, key)) return m->e[i].value;
    return NULL;
}

/* 0 and *out on success, -1 when the key is missing or its value is not one integer */
static int mf_manifest_int(const mf_manifest* m, const char* key, long long* out) {
    const char* v = mf_manifest_get(m, key);
    char* end;
    if (!v) return -1;
    *out = strtoll(v, &end, 10);
    return (end == v || *end) ? -1 : 0;
}

#endif /* MF_MANIFEST_READER_H */
