// record_swap_ref.cpp — the reference's own answers on NFCRecord::SwapRowInfo, for
// tests/golden/record_swap.json.  The script of tests/record_swap_model.py (golden_script(): REC / OBJ /
// INIT lines, then windows of SwapRowInfo calls among SetObject / SetInt / Remove / AddRow / Clear calls
// with FindObject / FindInt / QueryRow / GetObject calls between them) is replayed on the reference's
// NFCRecord objects (compiled from the reference tree where it lies; see
// tests/golden/gen_record_swap_golden.py).  The reference applies a call at once, so the frame line
// "X" does nothing here.  Every call line prints
//   A <k> <ret> : <list>
// ret the call's return value (a bool as 0 / 1, GetObject 0), list the find's rows, QueryRow's cells
// (an NFGUID as head then data, the others as uint64 bit patterns) or GetObject's head and data — and
// before it one line per event the record's hook received during the call,
//   E <k> <op> <row> <col> <old head> <old data> <new head> <new data>
// op 0 Update, 1 Add, 2 Del, 3 Cover, 4 Swap (row the origin, col the target row); an int / f64 value
// as head 0 and its bit pattern, a row event's as zeros.  An unknown object or record answers -1 / 0
// (there is no NFCRecord to ask).  TEST INFRASTRUCTURE, run by hand on a machine that has the reference
// tree.
//
// usage: record_swap_ref <script.txt>
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

static NFGUID guid_of(const std::string& tok) {
    const size_t c = tok.find(':');
    return NFGUID((NFINT64)strtoll(tok.substr(0, c).c_str(), nullptr, 10), (NFINT64)strtoll(tok.c_str() + c + 1, nullptr, 10));
}

static void add_value(NFCDataList& l, char type, const std::string& tok) {
    if (type == 'I') l.Add((NFINT64)strtoll(tok.c_str(), nullptr, 10));
    else if (type == 'F') l.Add(strtod(tok.c_str(), nullptr));
    else l.Add(guid_of(tok));
}

static int g_call = 0;  // the call the hook's events belong to

static void print_value(const NFIDataList::TData& v) {
    unsigned long long h = 0, d = 0;
    if (v.GetType() == TDATA_OBJECT) {
        h = (unsigned long long)v.GetObject().nHead64;
        d = (unsigned long long)v.GetObject().nData64;
    } else if (v.GetType() == TDATA_INT) {
        d = (unsigned long long)v.GetInt();
    } else if (v.GetType() == TDATA_FLOAT) {
        const double x = v.GetFloat();
        memcpy(&d, &x, 8);
    }
    printf(" %lld %lld", (long long)h, (long long)d);
}

static int on_record(const NFGUID&, const RECORD_EVENT_DATA& e, const NFIDataList::TData& o, const NFIDataList::TData& n) {
    int op = -1;
    switch (e.nOpType) {
    case RECORD_EVENT_DATA::Update: op = 0; break;
    case RECORD_EVENT_DATA::Add: op = 1; break;
    case RECORD_EVENT_DATA::Del: op = 2; break;
    case RECORD_EVENT_DATA::Cover: op = 3; break;
    case RECORD_EVENT_DATA::Swap: op = 4; break;
    default: break;
    }
    printf("E %d %d %d %d", g_call, op, e.nRow, e.nCol);
    print_value(o);
    print_value(n);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::vector<RecDef> defs;
    std::vector<std::vector<std::shared_ptr<NFCRecord>>> objs;
    NFCDataList last;
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
                        else if (c == 'F') types->Add(0.0);
                        else types->Add(NFGUID());
                        tags->Add("");
                    }
                    auto rec = std::make_shared<NFCRecord>(NFGUID(7, o + 1), d.name, types, tags, d.rows);
                    rec->AddRecordHook(RECORD_EVENT_FUNCTOR_PTR(new RECORD_EVENT_FUNCTOR(on_record)));
                    objs.back().push_back(rec);
                }
            }
            continue;
        }
        if (op == "X") continue;
        const int o = atoi(f[1].c_str()), r = atoi(f[2].c_str());
        const bool known = o >= 0 && o < (int)objs.size() && r >= 0 && r < (int)defs.size();
        NFCRecord* rec = known ? objs[o][r].get() : nullptr;
        long long ret = 0;
        std::vector<unsigned long long> lst;
        if (op == "INIT" || op == "AR") {
            if (!known) {
                ret = -1;
            } else if (f.size() > 4) {
                NFCDataList v;
                for (size_t c = 0; c + 4 < f.size() && c < defs[r].types.size(); c++) add_value(v, defs[r].types[c], f[4 + c]);
                ret = rec->AddRow(atoi(f[3].c_str()), v);
            } else {
                ret = rec->AddRow(atoi(f[3].c_str()));
            }
        } else if (op == "SO") {
            ret = known && rec->SetObject(atoi(f[3].c_str()), atoi(f[4].c_str()), guid_of(f[5]));
        } else if (op == "SI") {
            ret = known && rec->SetInt(atoi(f[3].c_str()), atoi(f[4].c_str()), (NFINT64)strtoll(f[5].c_str(), nullptr, 10));
        } else if (op == "RM") {
            ret = known && rec->Remove(atoi(f[3].c_str()));
        } else if (op == "CL") {
            ret = known && rec->Clear();
        } else if (op == "SW") {
            ret = known && rec->SwapRowInfo(atoi(f[3].c_str()), atoi(f[4].c_str()));
        } else if (op == "QR") {
            NFCDataList row;
            const bool ok = known && rec->QueryRow(atoi(f[3].c_str()), row);
            ret = ok ? 1 : 0;
            for (int c = 0; ok && c < row.GetCount(); c++) {
                if (row.Type(c) == TDATA_OBJECT) {
                    lst.push_back((unsigned long long)row.Object(c).nHead64);
                    lst.push_back((unsigned long long)row.Object(c).nData64);
                } else if (row.Type(c) == TDATA_INT) {
                    lst.push_back((unsigned long long)row.Int(c));
                } else {
                    const double d = row.Float(c);
                    unsigned long long b;
                    memcpy(&b, &d, 8);
                    lst.push_back(b);
                }
            }
        } else if (op == "GO") {
            const NFGUID g = known ? rec->GetObject(atoi(f[3].c_str()), atoi(f[4].c_str())) : NFGUID();
            lst.push_back((unsigned long long)g.nHead64);
            lst.push_back((unsigned long long)g.nData64);
        } else {
            if (op.back() != '+') last.Clear();
            const int col = atoi(f[3].c_str());
            if (!known) {
                ret = -1;
            } else if (op[1] == 'O') {
                ret = rec->FindObject(col, guid_of(f[4]), last);
            } else if (op[1] == 'I') {
                ret = rec->FindInt(col, (NFINT64)strtoll(f[4].c_str(), nullptr, 10), last);
            } else {
                NFCDataList var;
                for (int e = 0; e < atoi(f[4].c_str()); e++) add_value(var, f[5 + 2 * e][0], f[6 + 2 * e]);
                ret = rec->FindRowByColValue(col, var, last);
            }
            for (int i = 0; i < last.GetCount(); i++) lst.push_back((unsigned long long)last.Int(i));
        }
        printf("A %d %lld :", g_call, ret);
        for (unsigned long long x : lst) printf(" %llu", x);
        printf("\n");
        g_call++;
    }
    return 0;
}
