// enter_snapshot_ref.cpp — the reference's own enter payloads, for tests/golden/enter_snapshot.json.
// The script of tests/enter_snapshot_model.py (golden_script(): PROP / REC / OBJ lines, then windows of
// SetProperty* and record calls with snapshot lines "S <obj> <view>" between them) is replayed on the
// reference's NFCPropertyManager / NFCRecordManager objects (compiled from the reference tree where it
// lies; see tests/golden/gen_enter_snapshot_golden.py).  A snapshot walks First / Next with Changed(),
// GetPublic() / GetPrivate(), IsUsed and GetInt / GetFloat / GetObject as
// NFCGameServerNet_ServerModule::OnPropertyEnter (:289-375) and OnRecordEnter / OnRecordEnterPack
// (:402-470, :495-527) do, and prints names and bit patterns:
//   V <k> <n props> <n records>
//   P <name> <bits> [<head>]          (an object property: its data half, then its head half)
//   R <name> <used mask> : <cells, used rows ascending x columns>
// the format of tests/cpp/enter_snapshot_plugin.cpp.  The reference applies a call at once, so the
// frame line "X" does nothing here.  TEST INFRASTRUCTURE, run by hand on a machine that has the
// reference tree.
//
// usage: enter_snapshot_ref <script.txt>
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
#include "NFComm/NFCore/NFCPropertyManager.h"
#include "NFComm/NFCore/NFCRecordManager.h"

struct PropDef {
    std::string name;
    char type;
    int flags;
};
struct RecDef {
    std::string name, types;
    int rows, flags;
};
struct Obj {
    std::shared_ptr<NFCPropertyManager> props;
    std::shared_ptr<NFCRecordManager> recs;
};

static uint64_t dbits(double d) {
    uint64_t b;
    memcpy(&b, &d, 8);
    return b;
}

static void add_value(NFCDataList& l, char type, const std::string& tok) {
    if (type == 'I') l.Add((NFINT64)strtoll(tok.c_str(), nullptr, 10));
    else l.Add(strtod(tok.c_str(), nullptr));
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::vector<PropDef> pdefs;
    std::vector<RecDef> rdefs;
    std::vector<Obj> objs;
    int k = 0;
    std::string ln;
    while (std::getline(in, ln)) {
        std::istringstream ss(ln);
        std::vector<std::string> f;
        for (std::string t; ss >> t;) f.push_back(t);
        if (f.empty()) continue;
        const std::string& op = f[0];
        if (op == "PROP") {
            pdefs.push_back({f[1], f[2][0], atoi(f[3].c_str())});
            continue;
        }
        if (op == "REC") {
            rdefs.push_back({f[1], f[3], atoi(f[2].c_str()), atoi(f[4].c_str())});
            continue;
        }
        if (op == "OBJ") {
            for (int o = 0; o < atoi(f[1].c_str()); o++) {
                const NFGUID self(7, o + 1);
                Obj x{std::make_shared<NFCPropertyManager>(self), std::make_shared<NFCRecordManager>(self)};
                for (auto& d : pdefs) {
                    NF_SHARE_PTR<NFIProperty> p = x.props->AddProperty(
                        self, d.name, d.type == 'I' ? TDATA_INT : d.type == 'F' ? TDATA_FLOAT : TDATA_OBJECT);
                    p->SetPublic((d.flags & 1) != 0);
                    p->SetPrivate((d.flags & 2) != 0);
                    p->SetUpload((d.flags & 4) != 0);
                }
                for (auto& d : rdefs) {
                    NF_SHARE_PTR<NFIDataList> types(new NFCDataList()), tags(new NFCDataList());
                    for (char c : d.types) {
                        if (c == 'I') types->Add((NFINT64)0);
                        else types->Add(0.0);
                        tags->Add("");
                    }
                    NF_SHARE_PTR<NFIRecord> r = x.recs->AddRecord(self, d.name, types, tags, d.rows);
                    r->SetPublic((d.flags & 1) != 0);
                    r->SetPrivate((d.flags & 2) != 0);
                    r->SetUpload((d.flags & 4) != 0);
                }
                objs.push_back(x);
            }
            continue;
        }
        if (op == "X") continue;
        Obj& x = objs[(size_t)atoi(f[1].c_str())];
        if (op == "SI") {
            x.props->SetPropertyInt(f[2], (NFINT64)strtoll(f[3].c_str(), nullptr, 10));
        } else if (op == "SF") {
            x.props->SetPropertyFloat(f[2], strtod(f[3].c_str(), nullptr));
        } else if (op == "SO") {
            x.props->SetPropertyObject(f[2], NFGUID((NFINT64)strtoll(f[3].c_str(), nullptr, 10),
                                                    (NFINT64)strtoll(f[4].c_str(), nullptr, 10)));
        } else if (op == "S") {
            const bool priv = f[2] == "1";
            std::vector<std::string> out;
            int np = 0, nr = 0;
            // OnPropertyEnter (:289-375)
            NF_SHARE_PTR<NFIProperty> p = x.props->First();
            while (p) {
                if (p->Changed() && (priv ? p->GetPrivate() : p->GetPublic())) {
                    char b[160];
                    b[0] = 0;
                    switch (p->GetType()) {
                        case TDATA_INT:
                            snprintf(b, sizeof b, "P %s %llu", p->GetKey().c_str(), (unsigned long long)(uint64_t)p->GetInt());
                            break;
                        case TDATA_FLOAT:
                            snprintf(b, sizeof b, "P %s %llu", p->GetKey().c_str(), (unsigned long long)dbits(p->GetFloat()));
                            break;
                        case TDATA_OBJECT:
                            snprintf(b, sizeof b, "P %s %llu %llu", p->GetKey().c_str(),
                                     (unsigned long long)(uint64_t)p->GetObject().nData64,
                                     (unsigned long long)(uint64_t)p->GetObject().nHead64);
                            break;
                        default:
                            break;
                    }
                    if (b[0]) {
                        out.push_back(b);
                        np++;
                    }
                }
                p = x.props->Next();
            }
            // OnRecordEnter (:495-527) and OnRecordEnterPack (:402-470)
            NF_SHARE_PTR<NFIRecord> r = x.recs->First();
            while (r) {
                if (priv ? r->GetPrivate() : r->GetPublic()) {
                    uint64_t used = 0;
                    std::string cells;
                    for (int i = 0; i < r->GetRows(); i++) {
                        if (!r->IsUsed(i)) continue;
                        used |= 1ull << i;
                        for (int j = 0; j < r->GetCols(); j++) {
                            const uint64_t v = r->GetColType(j) == TDATA_INT ? (uint64_t)r->GetInt(i, j) : dbits(r->GetFloat(i, j));
                            cells += " " + std::to_string((unsigned long long)v);
                        }
                    }
                    out.push_back("R " + r->GetName() + " " + std::to_string((unsigned long long)used) + " :" + cells);
                    nr++;
                }
                r = x.recs->Next();
            }
            printf("V %d %d %d\n", k++, np, nr);
            for (auto& s : out) printf("%s\n", s.c_str());
        } else {
            NF_SHARE_PTR<NFIRecord> rec = x.recs->GetElement(f[2]);
            if (!rec) return 3;
            const RecDef* d = nullptr;
            for (auto& rd : rdefs)
                if (rd.name == f[2]) d = &rd;
            if (op == "AR") {
                if (f.size() > 4) {
                    NFCDataList v;
                    for (size_t c = 0; c + 4 < f.size(); c++) add_value(v, d->types[c], f[4 + c]);
                    rec->AddRow(atoi(f[3].c_str()), v);
                } else {
                    rec->AddRow(atoi(f[3].c_str()));
                }
            } else if (op == "RI") {
                rec->SetInt(atoi(f[3].c_str()), atoi(f[4].c_str()), (NFINT64)strtoll(f[5].c_str(), nullptr, 10));
            } else if (op == "RM") {
                rec->Remove(atoi(f[3].c_str()));
            } else if (op == "CL") {
                rec->Clear();
            }
        }
    }
    return 0;
}
