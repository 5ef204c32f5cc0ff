// record_find_ref.cpp — the reference's own answers to the record finds, for tests/golden/record_find.json.
// The script of tests/record_find_model.py (golden_script(): REC / OBJ / INIT lines, then windows of
// SetRecordInt / Remove / AddRow / ClearRecord calls with FindInt / FindFloat / FindRowByColValue /
// QueryRow calls between them) is replayed on the reference's NFCRecord objects (compiled from the
// reference tree where it lies; see tests/golden/gen_record_find_golden.py).  The reference applies a
// call at once, so the frame line "X" does nothing here.  Every find / QueryRow prints one line,
//   A <k> <ret> : <rows of varResult>          (QR: <0 | 1> : the row's cells as uint64 bit patterns)
// the format of tests/cpp/record_find_plugin.cpp.  An unknown object or record answers -1 (there is no
// NFCRecord to ask).  TEST INFRASTRUCTURE, run by hand on a machine that has the reference tree.
//
// usage: record_find_ref <script.txt>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "NFComm/NFCore/NFCDataList.h"
#include "NFComm/NFCore/NFCRecord.h"

struct RecDef {
    std::string name, types;
    int rows;
};

static void add_value(NFCDataList& l, char type, const std::string& tok) {
    if (type == 'I') l.Add((NFINT64)strtoll(tok.c_str(), nullptr, 10));
    else l.Add(strtod(tok.c_str(), nullptr));
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::vector<RecDef> defs;
    std::vector<std::vector<std::shared_ptr<NFCRecord>>> objs;
    NFCDataList last;
    int k = 0;
    std::string ln;
    while (std::getline(in, ln)) {
        std::istringstream ss(ln);
        std::vector<std::string> f;
        for (std::string t; ss >> t;) f.push_back(t);
        if (f.empty()) continue;
        const std::string& op = f[0];
        if (op == "REC") {
            defs.push_back({f[1], f[3], atoi(f[2].c_str())});
            continue;
        }
        if (op == "OBJ") {
            for (int o = 0; o < atoi(f[1].c_str()); o++) {
                objs.emplace_back();
                for (auto& d : defs) {
                    NF_SHARE_PTR<NFIDataList> types(new NFCDataList()), tags(new NFCDataList());
                    for (char c : d.types) {
                        if (c == 'I') types->Add((NFINT64)0);
                        else types->Add(0.0);
                        tags->Add("");
                    }
                    objs.back().push_back(std::make_shared<NFCRecord>(NFGUID(7, o + 1), d.name, types, tags, d.rows));
                }
            }
            continue;
        }
        if (op == "X") continue;
        const int o = atoi(f[1].c_str()), r = atoi(f[2].c_str());
        const bool known = o >= 0 && o < (int)objs.size() && r >= 0 && r < (int)defs.size();
        NFCRecord* rec = known ? objs[o][r].get() : nullptr;
        if (op == "INIT" || op == "AR") {
            if (f.size() > 4) {
                NFCDataList v;
                for (size_t c = 0; c + 4 < f.size(); c++) add_value(v, defs[r].types[c], f[4 + c]);
                rec->AddRow(atoi(f[3].c_str()), v);
            } else {
                rec->AddRow(atoi(f[3].c_str()));
            }
        } else if (op == "SI") {
            rec->SetInt(atoi(f[3].c_str()), atoi(f[4].c_str()), (NFINT64)strtoll(f[5].c_str(), nullptr, 10));
        } else if (op == "RM") {
            rec->Remove(atoi(f[3].c_str()));
        } else if (op == "CL") {
            rec->Clear();
        } else if (op == "QR") {
            NFCDataList row;
            const bool ok = known && rec->QueryRow(atoi(f[3].c_str()), row);
            printf("A %d %d :", k++, ok ? 1 : 0);
            for (int c = 0; ok && c < row.GetCount(); c++) {
                uint64_t b;
                if (row.Type(c) == TDATA_INT) {
                    b = (uint64_t)row.Int(c);
                } else {
                    const double d = row.Float(c);
                    memcpy(&b, &d, 8);
                }
                printf(" %llu", (unsigned long long)b);
            }
            printf("\n");
        } else {
            if (op.back() != '+') last.Clear();
            const int col = atoi(f[3].c_str());
            int ret = -1;
            if (!known) {
                ret = -1;
            } else if (op[1] == 'I') {
                ret = rec->FindInt(col, (NFINT64)strtoll(f[4].c_str(), nullptr, 10), last);
            } else if (op[1] == 'F') {
                ret = rec->FindFloat(col, strtod(f[4].c_str(), nullptr), last);
            } else {
                NFCDataList var;
                for (int e = 0; e < atoi(f[4].c_str()); e++) add_value(var, f[5 + 2 * e][0], f[6 + 2 * e]);
                ret = rec->FindRowByColValue(col, var, last);
            }
            printf("A %d %d :", k++, ret);
            for (int i = 0; i < last.GetCount(); i++) printf(" %lld", (long long)last.Int(i));
            printf("\n");
        }
    }
    return 0;
}
